#!/usr/bin/env python
"""Anchored sampling (RQTransformer.anchor: the quantiser's soft-code term of an encoded image folded into the logits inside the engine)
at the 1.4B shape: E 1536, 24 heads, 42 body + 6 head layers, 8 x 8 x 4 codes, vocabulary 16384, code width 256
(oracle.configs.RQT_IN_1400M, random weights), top_k 1024 / top_p 0.95, captured graphs.  Time per call of the AR pass, device events, one
warm-up call per case (it captures the graphs), the two cases alternated in one process, B in {8, 64, 500}:

  sample, B images                 the plain call: what the user paid before
  sample inside anchor(z, w), B    three more launches per head step: the residual of the B images (B x 256), the quantiser's fp32-MFMA
                                   distance kernel (B x 16384 x 256) and the fold (2 row reads, 1 row write per image)

anchored / plain is the price of the anchor; the difference divided by the H * W * D head steps of a call is its cost per head step.
Nothing is asserted.  Arguments: the batch sizes (default: 8 64 500); --out FILE: where the lines are written besides stdout (default:
profiles/anchored_sampling_bench.txt)."""
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
DIM = 256


class Aux:
    """model_aux: one codebook shared by the depths, its norms, and features that already have the code shape"""

    def __init__(self, V, depth):
        cb = 0.1 * torch.randn((V, DIM), device=dev)
        norms = _native.rq_code_norms(cb)

        class Q:
            @staticmethod
            def codebook_list():
                return [cb] * depth

            @staticmethod
            def _norm_list():
                return [norms] * depth

            @staticmethod
            def to_code_shape(x):
                return x
        self.quantizer = Q


def time_ms(fns, reps):
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


def main(batches, out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'rqt_anchor.hip', 'quantize.hip', 'engine_rqt.hip'))}")
    cfg = cfgs.RQT_IN_1400M
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    (H, W, D) = cfg['block_size']
    aux = Aux(16384, D)
    vc = max(cfg['vocab_size_cond'], 1)
    steps = H * W * D
    for B in batches:
        part = torch.zeros((B, H, W, D), dtype=torch.long, device=dev)
        cond = torch.randint(0, vc, (B, 1), device=dev)
        z = 0.15 * torch.randn((B, H, W, DIM), device=dev)

        def anchored():
            with ar.anchor(z, 1.0):
                return ar.sample(part, aux, cond=cond, **KW)
        out = time_ms({f'sample, {B} images': lambda: ar.sample(part, aux, cond=cond, **KW),
                       f'sample inside anchor(z, 1.0), {B} images': anchored}, reps=5 if B <= 64 else 3)
        (plain, anc) = out.values()
        say(f'== B = {B}, 1.4B shape, {H} x {W} x {D}, top_k 1024 / top_p 0.95, graphs')
        for k, (med, lo) in out.items():
            say(f'  {k:44s} {med:9.2f} ms per call (min {lo:9.2f})')
        say(f'  anchored / plain: {anc[0] / plain[0]:.3f} (medians), {anc[1] / plain[1]:.3f} (minima); '
            f'difference per head step {1e3 * (anc[0] - plain[0]) / steps:+.2f} us (medians), {1e3 * (anc[1] - plain[1]) / steps:+.2f} us (minima)')
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, 'profiles', 'anchored_sampling_bench.txt')
    if '--out' in args:
        i = args.index('--out')
        out_path = args[i + 1]
        del args[i:i + 2]
    main([int(a) for a in args] or [8, 64, 500], out_path)
