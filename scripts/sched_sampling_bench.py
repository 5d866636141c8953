#!/usr/bin/env python
"""Sampling schedules over positions and depths: what a scheduled call costs (rqamd_rqt_sample_schedule, RQTransformer.schedule()).

One sample() / sample_guided() of the 1.4B shape (oracle.configs.RQT_IN_1400M, random weights, 8 x 8 x 4 codes, vocabulary 16384,
captured graphs) at 64 / 500 / 2048 images, top_k = 1024 / top_p = 0.95, one process, device events around the whole call (the AR
pass and the host work in front of it), one warm-up each, the configurations alternated, medians and minima of `reps` rounds:

  (a)  the per-image call, the same values in every row (temperature / top_k / top_p as (B,) tensors); timed twice per round, as (a)
       and (a'): the spread between the two is the margin the other lines are read against
  (b)  the shared schedule, (H, W) tensors that hold those values everywhere: one small table, the same launches as (a)
  (c)  a per-image schedule, (B, H, W, D) tensors with them: B * H * W * D entries per table, filled on the host before the pass
  (d0) sample_guided at the constant scale 4
  (d1) sample_guided under a guidance ramp 1 -> 4 over the positions (position_ramp)

(b), (c) and (d1) issue the launches of (a) and (d0) with the scheduled sampler kernels, so they are held against those.  Any excess
over the margin is reported; nothing is asserted about the times.  (b) and (c) must return the codes of (a), which is asserted.

usage: sched_sampling_bench.py [--batches 64,500,2048] [--reps 5] [--out FILE]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'rq-vae-transformer_amd'))
import torch  # noqa: E402
from rqvae import _native  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device('cuda', 0)
V, TOP_K, TOP_P = 16384, 1024, 0.95
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def time_all(fns, reps):
    """fns: name -> callable; one warm-up each, then alternated; returns name -> (median, min, max) ms per call"""
    for k, f in fns.items():
        f()
        torch.cuda.synchronize()
        print(f'  warmed up {k.strip()}', flush=True)
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            res[k].append(timed(f))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in res.items()}


class Aux:
    def __init__(self, depth):
        t = torch.randn((V, 256), device=dev)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def scheduled(ar, fn, **sched):
    def f():
        with ar.schedule(**sched):
            return fn()
    return f


def run(ar, aux, cfg, B, reps):
    (H, W, D) = cfg['block_size']
    part = torch.zeros((B, H, W, D), dtype=torch.long, device=dev)
    cond = torch.randint(0, max(cfg['vocab_size_cond'], 1), (B, 1), device=dev)
    uncond = (cond + 1) % max(cfg['vocab_size_cond'], 2)
    ar._draw_rng = lambda device, n: (1234, 8)              # every configuration draws from the same counters
    rows = dict(temperature=torch.ones(B, device=dev), top_k=torch.full((B,), TOP_K, device=dev), top_p=torch.full((B,), TOP_P, device=dev))
    shared = dict(temperature=torch.ones((H, W)), top_k=torch.full((H, W), TOP_K), top_p=torch.full((H, W), TOP_P))
    image = dict(temperature=torch.ones((B, H, W, D)), top_k=torch.full((B, H, W, D), TOP_K), top_p=torch.full((B, H, W, D), TOP_P))
    plain = lambda: ar.sample(part, aux, cond=cond)
    per_image = lambda: ar.sample(part, aux, cond=cond, **rows)
    guided = lambda **kw: ar.sample_guided(part, aux, cond=cond, uncond=uncond, top_k=TOP_K, top_p=TOP_P, **kw)
    fns = {'(a)  per-image call': per_image,
           '(b)  shared schedule': scheduled(ar, plain, **shared),
           '(c)  per-image schedule': scheduled(ar, plain, **image),
           "(a') per-image call again": per_image,
           '(d0) guided, scale 4': lambda: guided(guidance_scale=4.0),
           '(d1) guided, ramp 1 -> 4': scheduled(ar, guided, guidance_scale=ar.position_ramp(1.0, 4.0))}
    a = fns['(a)  per-image call']()
    same = [bool(torch.equal(fns[k](), a)) for k in ('(b)  shared schedule', '(c)  per-image schedule')]
    assert all(same), 'a constant schedule does not return the per-image call\'s codes'
    res = time_all(fns, reps)
    say(f'== B = {B}: 1.4B shape, {H} x {W} x {D}, top_k {TOP_K} / top_p {TOP_P}, graphs; ms per call, medians of {reps} (min .. max); '
        f'(b), (c) return the codes of (a): {all(same)}')
    base, again, g0 = res['(a)  per-image call'], res["(a') per-image call again"], res['(d0) guided, scale 4']
    margin = max(abs(again[0] - base[0]), base[2] - base[1], again[2] - again[1])
    for k, (med, lo, hi) in res.items():
        ref = g0 if k.startswith('(d') else base
        say(f'  {k:28s} {med:10.2f} ({lo:10.2f} .. {hi:10.2f})   {med - ref[0]:+8.2f} ms = {100 * (med / ref[0] - 1):+6.2f} % of {"(d0)" if ref is g0 else "(a)"}')
    say(f"  margin (spread of (a) and (a')): {margin:.2f} ms = {100 * margin / base[0]:.2f} %")
    for k in ('(b)  shared schedule', '(c)  per-image schedule'):
        over = res[k][0] - base[0] - margin
        say(f'  {k.strip()}: ' + (f'{over:.2f} ms over the margin' if over > 0 else 'within the margin'))


if __name__ == '__main__':
    args = sys.argv[1:]
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    batches = [int(b) for b in opt('--batches', '64,500,2048').split(',')]
    reps = int(opt('--reps', '5'))
    from oracle import configs as cfgs
    from rqvae.models.rqtransformer import RQTransformer
    cfg = cfgs.RQT_IN_1400M
    say(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'engine_rqt.hip'))}")
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    aux = Aux(cfg['block_size'][2])
    for B in batches:
        run(ar, aux, cfg, B, reps)
    out = opt('--out', None)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            fh.write('scripts/sched_sampling_bench.py\n' + '\n'.join(lines) + '\n')
