#!/usr/bin/env python
"""Completion calls (RQTransformer.sample(start_loc=...)) with the given prefix stepped and filled in one pass, at the 1.4B shape: E 1536,
24 heads, 42 body + 6 head layers, 8 x 8 x 4 codes, vocabulary 16384 (oracle.configs.RQT_IN_1400M, random weights), top_k 1024 /
top_p 0.95, captured graphs.  Time per call at start_loc = (4, 0) (32 given positions, 32 drawn) and (7, 7) (63 given, one drawn), device
events, one warm-up call per case, prefix_mode = 'stepped' and 'one_pass' alternated in one process, medians of 5.

The stepped prefix streams the body weights once per given position, whatever the batch; the one-pass prefix once per chunk of
fwd.chunk_rows = 4096 rows (images x tokens).  At thousands of images a stepped step already amortises the weights over its rows, so
the sweep shows where the one-pass prefix stops winning.

Optional arguments: the batch sizes (default: 8 64 500 2048)."""
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


def main(batches):
    print(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'engine_rqt.hip'))}")
    cfg = cfgs.RQT_IN_1400M
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    aux = Aux(16384, 4)
    (H, W, D) = cfg['block_size']

    def call(mode, part, cond, start):
        ar.prefix_mode = mode
        return ar.sample(part, aux, cond=cond, start_loc=start, **KW)
    rows = []
    for B in batches:
        part = torch.randint(0, 16384, (B, H, W, D), device=dev)
        cond = torch.zeros((B, 1), device=dev, dtype=torch.long)
        print(f'== {B} images, 1.4B shape, {H} x {W} x {D}, top_k 1024 / top_p 0.95, graphs, medians of {REPS}')
        for start in ((H // 2, 0), (H - 1, W - 1)):
            n0 = start[0] * W + start[1]
            out = time_ms({m: (lambda m=m: call(m, part, cond, start)) for m in ('stepped', 'one_pass')})
            (st, st_lo), (op, op_lo) = out['stepped'], out['one_pass']
            chunks = -(-B // max(1, min(B, 4096 // n0)))
            print(f'  start_loc {start}: {n0:2d} given positions  stepped {st:9.2f} ms (min {st_lo:9.2f})  one-pass {op:9.2f} ms (min {op_lo:9.2f})'
                  f'  {st / op:5.2f} x  [{B * n0} prefix rows in {chunks} chunk(s)]')
            rows.append((B, start, st / op))
    print('== stepped / one-pass per call (above 1: the one-pass prefix wins)')
    for B, start, r in rows:
        print(f'  {B:5d} images, start_loc {start}: {r:5.2f} x')
    lost = [(B, start) for B, start, r in rows if r < 1.0]
    print('  crossover: ' + (f'the one-pass prefix loses at {lost}' if lost else 'none inside the sweep: the one-pass prefix wins at every batch size'))
    ar.prefix_mode = 'stepped'


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [8, 64, 500, 2048])
