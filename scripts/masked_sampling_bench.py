#!/usr/bin/env python
"""Masked sampling (RQTransformer.sample(keep_mask=...)) at the 1.4B shape: E 1536, 24 heads, 42 body + 6 head layers, 8 x 8 x 4 codes,
vocabulary 16384 (oracle.configs.RQT_IN_1400M, random weights), top_k 1024 / top_p 0.95, captured graphs.  Time per batch at 64 and 500
images, device events, one warm-up call per case (it captures the graphs), the cases alternated in one process:

  unmasked                      sample() as it was
  mask, nothing kept            every position active, every sampler workgroup draws: must be level with unmasked
  left half of every row kept   outpainting: every position runs its body step, half of them their head steps too
  top half kept                 a raster prefix as a mask; next to it start_loc=(4, 0), the same work
  depths 2 and 3 redrawn        depth refinement: every position active, two of four draws per position

Optional arguments: the batch sizes (default: 64 500)."""
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
    none = torch.zeros((H, W), dtype=torch.bool, device=dev)
    left = none.clone()
    left[:, :W // 2] = True
    top = none.clone()
    top[:H // 2] = True
    fine = torch.zeros((H, W, D), dtype=torch.bool, device=dev)
    fine[..., :2] = True
    for B in batches:
        part = torch.randint(0, 16384, (B, H, W, D), device=dev)
        cond = torch.zeros((B, 1), device=dev, dtype=torch.long)
        out = time_ms({
            'unmasked': lambda: ar.sample(part, aux, cond=cond, **KW),
            'mask, nothing kept': lambda: ar.sample(part, aux, cond=cond, keep_mask=none, **KW),
            'left half of every row kept': lambda: ar.sample(part, aux, cond=cond, keep_mask=left, **KW),
            'top half kept': lambda: ar.sample(part, aux, cond=cond, keep_mask=top, **KW),
            'start_loc=(4, 0)': lambda: ar.sample(part, aux, cond=cond, start_loc=(H // 2, 0), **KW),
            'depths 2 and 3 redrawn': lambda: ar.sample(part, aux, cond=cond, keep_mask=fine, **KW),
        })
        base = out['unmasked'][0]
        print(f'== {B} images, 1.4B shape, {H} x {W} x {D}, top_k 1024 / top_p 0.95, graphs')
        for k, (med, lo) in out.items():
            print(f'  {k:30s} {med:9.2f} ms per batch (min {lo:9.2f})  {med / base:5.2f} x unmasked')


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [64, 500])
