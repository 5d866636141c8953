#!/usr/bin/env python
"""Masked sampling calls (RQTransformer.sample(keep_mask=...)) with their interior kept runs stepped and filled in one pass, at the 1.4B
shape: E 1536, 24 heads, 42 body + 6 head layers, 8 x 8 x 4 codes, vocabulary 16384 (oracle.configs.RQT_IN_1400M, random weights),
top_k 1024 / top_p 0.95, captured graphs.  Masks over the 8 x 8 map, the same for every image:

  left4   columns 0 .. 3 of every row kept     a run of 4 positions in front of every row's drawn half
  left7   columns 0 .. 6 of every row kept     runs of 7 positions, one drawn position a row
  hole    a 4 x 4 hole in the middle drawn     a leading run of 18, rim runs of 4 between the hole's rows, the rest is never run
  bands   rows 0 - 2 and 5 - 7 kept            a leading run of 24; rows 5 - 7 lie behind the last drawn position and are never run

Time per call, device events, one warm-up call per case; kept_run_mode = 'stepped' and 'one_pass' alternated in one process with
prefix_mode off ('stepped') and on ('one_pass'), medians of 5.  A stepped kept position streams the body weights once, whatever the
batch; a run once per chunk of fwd.chunk_rows = 4096 rows (images x tokens).

Optional arguments: the batch sizes (default: 8 64 500)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'rq-vae-transformer_amd'))
import torch  # noqa: E402
from oracle import configs as cfgs  # noqa: E402
from rqvae import _native  # noqa: E402
from rqvae.models.rqtransformer import RQTransformer  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device('cuda', 0)
KW = dict(top_k=1024, top_p=0.95)
REPS = 5


class Aux:
    def __init__(self, V, depth):
        t = torch.randn((V, 256), device=dev)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def time_ms(fns, reps=REPS):
    """fns: name -> callable; one warm-up each, then alternated; returns name -> (median, min) ms per call"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            res[k].append(e0.elapsed_time(e1))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in res.items()}


def masks(H, W):
    m = {k: torch.zeros((H, W), dtype=torch.bool, device=dev) for k in ('left4', 'left7', 'hole', 'bands')}
    m['left4'][:, :W // 2] = True
    m['left7'][:, :W - 1] = True
    m['hole'][:] = True
    m['hole'][H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2] = False
    m['bands'][:3] = True
    m['bands'][5:] = True
    return m


def runs_of(mask, prefix_on):
    """(stepped kept positions, [run lengths]) of the call under the engine's rule"""
    flat = mask.flatten().tolist()
    last = max(i for i, k in enumerate(flat) if not k)
    n0 = 0
    while prefix_on and flat[n0]:
        n0 += 1
    runs, p = [], max(n0, 1)
    kept = sum(flat[n0:last])
    while p < last:
        if flat[p]:
            q = p
            while flat[q]:
                q += 1
            if q - p >= 2:
                runs.append(q - p)
            p = q
        else:
            p += 1
    return kept, runs


def main(batches):
    print(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_attn_extend.hip', 'rqt_kernels.hip', 'engine_rqt.hip'))}")
    cfg = cfgs.RQT_IN_1400M
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    aux = Aux(16384, 4)
    (H, W, D) = cfg['block_size']

    def call(prefix, mode, part, cond, mask):
        ar.prefix_mode, ar.kept_run_mode = prefix, mode
        return ar.sample(part, aux, cond=cond, keep_mask=mask, **KW)
    rows = []
    for B in batches:
        part = torch.randint(0, 16384, (B, H, W, D), device=dev)
        cond = torch.zeros((B, 1), device=dev, dtype=torch.long)
        print(f'== {B} images, 1.4B shape, {H} x {W} x {D}, top_k 1024 / top_p 0.95, graphs, medians of {REPS}')
        for name, mask in masks(H, W).items():
            for prefix in ('stepped', 'one_pass'):
                out = time_ms({m: (lambda m=m: call(prefix, m, part, cond, mask)) for m in ('stepped', 'one_pass')})
                (st, st_lo), (op, op_lo) = out['stepped'], out['one_pass']
                kept, runs = runs_of(mask, prefix == 'one_pass')
                print(f'  {name:6s} prefix_mode {prefix:8s}: stepped {st:9.2f} ms (min {st_lo:9.2f})  one-pass {op:9.2f} ms (min {op_lo:9.2f})'
                      f'  {st / op:5.2f} x  [{kept} kept positions behind the prefix, runs {runs}]')
                rows.append((B, name, prefix, st / op))
    print('== stepped / one-pass per call (above 1: the one-pass runs win)')
    for B, name, prefix, r in rows:
        print(f'  {B:5d} images, {name:6s} prefix_mode {prefix:8s}: {r:5.2f} x')
    lost = [(B, name, prefix) for B, name, prefix, r in rows if r < 1.0]
    print('  crossover: ' + (f'the one-pass runs lose at {lost}' if lost else 'none inside the sweep: the one-pass runs win or tie everywhere'))
    ar.prefix_mode = ar.kept_run_mode = 'stepped'


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [8, 64, 500])
