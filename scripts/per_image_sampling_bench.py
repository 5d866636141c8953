#!/usr/bin/env python
"""Per-image sampling parameters (tensor arguments of RQTransformer.sample / sample_guided, rqamd_rqt_sample_rows) at the 1.4B shape:
E 1536, 24 heads, 42 body + 6 head layers, 8 x 8 x 4 codes, vocabulary 16384 (oracle.configs.RQT_IN_1400M, random weights), captured
graphs.  Time per call (the AR pass), device events, one warm-up call per case (it captures the graphs), the cases alternated in one
process, medians of `reps` runs, B in {64, 500, 2048}:

  (a) scalar            sample(top_k=1024, top_p=0.95)
  (b) per-row, uniform  the same values in every row, given as (B,) tensors: the per-row kernels, every row in the register kernel's class
  (c) per-row, mixed    a third of the rows unfiltered, a third top-k 1024 only, a third top-k 1024 + top-p 0.95, interleaved

(b) is held against (a) of the same run: the per-row launch sequence is at most one launch longer per (position, depth) -- the three
per-row kernels against the register kernel and the general kernel's second pass -- and a dependent in-graph launch was measured at
1.53 us (README.md, round 4), which predicts 64 x 4 x 1.53 us = 0.4 ms per AR pass.

Then a sweep of four guidance scales over S images each: four scalar sample_guided calls (each new scale recaptures the guided graphs)
against one per-row call over the concatenated 4 S images.  Nothing is asserted.  Optional arguments: the batch sizes (default: 64 500
2048); the sweep runs at S = 64."""
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
TOP_K, TOP_P, V = 1024, 0.95, 16384
SCALES = (1.0, 2.0, 3.0, 5.0)


class Aux:
    def __init__(self, V, depth):
        t = torch.randn((V, 256), device=dev)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def time_ms(fns, reps=5):
    """fns: name -> callable; one warm-up each, then alternated; returns name -> (median, min) ms per call"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            res[k].append(timed(f))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in res.items()}


def main(batches, sweep_images=64):
    print(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'engine_rqt.hip'))}")
    cfg = cfgs.RQT_IN_1400M
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    aux = Aux(V, 4)
    (H, W, D) = cfg['block_size']
    vc = max(cfg['vocab_size_cond'], 1)
    for B in batches:
        part = torch.zeros((B, H, W, D), dtype=torch.long, device=dev)
        cond = torch.randint(0, vc, (B, 1), device=dev)
        ones = torch.ones(B, device=dev)
        third = torch.arange(B, device=dev) % 3
        uni = dict(temperature=ones, top_k=torch.full((B,), TOP_K, device=dev), top_p=torch.full((B,), TOP_P, device=dev))
        mixed = dict(temperature=ones, top_k=torch.where(third == 0, V, TOP_K), top_p=torch.where(third == 2, TOP_P, 1.0).float())
        out = time_ms({
            '(a) scalar': lambda: ar.sample(part, aux, cond=cond, top_k=TOP_K, top_p=TOP_P),
            '(b) per-row, uniform': lambda: ar.sample(part, aux, cond=cond, **uni),
            '(c) per-row, mixed thirds': lambda: ar.sample(part, aux, cond=cond, **mixed),
        })
        (a, b, c) = out.values()
        print(f'== B = {B}, 1.4B shape, {H} x {W} x {D}, top_k {TOP_K} / top_p {TOP_P}, graphs, medians of 5')
        for k, (med, lo) in out.items():
            print(f'  {k:28s} {med:9.2f} ms per call (min {lo:9.2f})')
        print(f'  (b) - (a): {b[0] - a[0]:+.2f} ms (medians), {b[1] - a[1]:+.2f} ms (minima); predicted +{H * W * D * 1.53e-3:.2f} ms for one more launch per (position, depth)')
        print(f'  (c) - (a): {c[0] - a[0]:+.2f} ms (medians), {c[1] - a[1]:+.2f} ms (minima)')
    # ---- a sweep of four guidance scales
    S = sweep_images
    part = torch.zeros((S, H, W, D), dtype=torch.long, device=dev)
    cond = torch.randint(0, vc, (S, 1), device=dev)
    uncond = (cond + vc // 2) % vc
    part4, cond4, uncond4 = torch.cat([part] * 4), torch.cat([cond] * 4), torch.cat([uncond] * 4)
    scales4 = torch.tensor([s for s in SCALES for _ in range(S)], device=dev)

    def four_scalar():
        for s in SCALES:
            ar.sample_guided(part, aux, cond=cond, uncond=uncond, guidance_scale=s, top_k=TOP_K, top_p=TOP_P)

    def one_per_row():
        ar.sample_guided(part4, aux, cond=cond4, uncond=uncond4, guidance_scale=scales4, top_k=TOP_K, top_p=TOP_P)
    out = time_ms({f'four scalar sample_guided calls, {S} images each': four_scalar,
                   f'one per-row sample_guided call, {4 * S} images': one_per_row}, reps=3)
    (four, one) = out.values()
    print(f'== sweep of guidance scales {SCALES}, {S} images per scale, top_k {TOP_K} / top_p {TOP_P}, graphs, medians of 3')
    for k, (med, lo) in out.items():
        print(f'  {k:52s} {med:9.2f} ms (min {lo:9.2f})')
    print(f'  four scalar calls / one per-row call: {four[0] / one[0]:.2f} (medians)')


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [64, 500, 2048])
