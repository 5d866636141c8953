#!/usr/bin/env python
"""Composed guidance (RQTransformer.extra_conds / sample_guided(negative=...): extra conditions folded into the guided logits inside the
engine) at the 1.4B shape: E 1536, 24 heads, 42 body + 6 head layers, 8 x 8 x 4 codes, vocabulary 16384 (oracle.configs.RQT_IN_1400M,
random weights), top_k 1024 / top_p 0.95, captured graphs.  Time per call, device events, one warm-up call per case (it captures the
graphs), the three cases alternated in one process, B in {32, 250, 1024}:

  composed, K = 1, B images     3B engine rows (cond, uncond, the negative prompt), one fold launch per head step (3 row reads, 2 row
                                writes per image), B sampler rows that read two rows of the fold's scratch
  sample, 3B images             the same GEMM and attention work, no fold, 3B sampler rows that read one logits row each
  sample_guided, B images       2B engine rows: what the user paid before the negative prompt

composed - plain over 3B rows, divided by the H * W * D head steps of a call, is the cost of the fold per head step net of the 2B
sampler rows the plain call runs in addition; composed / guided is the price of the negative prompt.  Nothing is asserted.  Optional
arguments: the batch sizes (default: 32 250 1024)."""
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


class Aux:
    def __init__(self, V, depth):
        t = torch.randn((V, 256), device=dev)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def time_ms(fns, reps=5):
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
    print(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'rqt_compose.hip', 'engine_rqt.hip'))}")
    cfg = cfgs.RQT_IN_1400M
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    aux = Aux(16384, 4)
    (H, W, D) = cfg['block_size']
    vc = max(cfg['vocab_size_cond'], 1)
    for B in batches:
        part = torch.zeros((B, H, W, D), dtype=torch.long, device=dev)
        part3 = torch.cat([part, part, part])
        cond = torch.randint(0, vc, (B, 1), device=dev)
        uncond = (cond + vc // 2) % vc
        neg = (cond + vc // 3) % vc
        cond3 = torch.cat([cond, uncond, neg])
        gk = dict(cond=cond, uncond=uncond, guidance_scale=3.0, **KW)
        out = time_ms({
            f'composed K = 1, {B} images (s = 3, w = -1.5)': lambda: ar.sample_guided(part, aux, negative=neg, negative_scale=1.5, **gk),
            f'sample, {3 * B} images': lambda: ar.sample(part3, aux, cond=cond3, **KW),
            f'sample_guided, {B} images (s = 3)': lambda: ar.sample_guided(part, aux, **gk),
        })
        (composed, plain, guided) = out.values()
        steps = H * W * D
        print(f'== B = {B}, 1.4B shape, {H} x {W} x {D}, top_k 1024 / top_p 0.95, graphs')
        for k, (med, lo) in out.items():
            print(f'  {k:44s} {med:9.2f} ms per call (min {lo:9.2f})')
        print(f'  composed / plain over 3B rows: {composed[0] / plain[0]:.3f} (medians), {composed[1] / plain[1]:.3f} (minima); '
              f'difference per head step {1e3 * (composed[0] - plain[0]) / steps:+.2f} us (medians), {1e3 * (composed[1] - plain[1]) / steps:+.2f} us (minima)')
        print(f'  composed / guided over B images: {composed[0] / guided[0]:.3f} (medians), {composed[1] / guided[1]:.3f} (minima)')


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [32, 250, 1024])
