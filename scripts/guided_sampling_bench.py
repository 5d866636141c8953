#!/usr/bin/env python
"""Guided sampling (RQTransformer.sample_guided, classifier-free guidance inside the engine) at the 1.4B shape: E 1536, 24 heads,
42 body + 6 head layers, 8 x 8 x 4 codes, vocabulary 16384 (oracle.configs.RQT_IN_1400M, random weights), top_k 1024 / top_p 0.95,
captured graphs.  Time per call, device events, one warm-up call per case (it captures the graphs), the two cases alternated in one
process, B in {32, 250, 1024}:

  sample_guided, B images       2B engine rows (images under cond, their twins under uncond), B sampler rows that read two logits rows
  sample, 2B images             the same GEMM and attention work, 2B sampler rows that read one logits row each

The expectation is a ratio near 1; nothing is asserted.  Optional arguments: the batch sizes (default: 32 250 1024)."""
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


def time_ms(fns, reps=3):
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
    vc = max(cfg['vocab_size_cond'], 1)
    for B in batches:
        part = torch.zeros((B, H, W, D), dtype=torch.long, device=dev)
        part2 = torch.cat([part, part])
        cond = torch.randint(0, vc, (B, 1), device=dev)
        uncond = (cond + vc // 2) % vc
        cond2 = torch.cat([cond, uncond])
        out = time_ms({
            f'sample_guided, {B} images (s = 3)': lambda: ar.sample_guided(part, aux, cond=cond, uncond=uncond, guidance_scale=3.0, **KW),
            f'sample, {2 * B} images': lambda: ar.sample(part2, aux, cond=cond2, **KW),
        })
        (guided, plain) = out.values()
        print(f'== B = {B}, 1.4B shape, {H} x {W} x {D}, top_k 1024 / top_p 0.95, graphs')
        for k, (med, lo) in out.items():
            print(f'  {k:36s} {med:9.2f} ms per call (min {lo:9.2f})')
        print(f'  guided / plain over 2B rows: {guided[0] / plain[0]:.3f} (medians), {guided[1] / plain[1]:.3f} (minima)')


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [32, 250, 1024])
