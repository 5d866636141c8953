#!/usr/bin/env python
"""Shared-prompt sampling (RQTransformer.shared_cond(n): n images per prompt on one cached text prefix) against the plain call with every
prompt repeated, on the two text-to-image shapes: txt3900m (E 2560, 40 heads, 42 + 6 layers, 64 text tokens; oracle.configs.RQT_TXT_3900M)
and the CC-3M shape (E 1280, 20 heads, 26 + 4 layers, 32 text tokens; RQT_CC3M_654M).  Random weights, 8 x 8 x 4 codes, top_k 1024 /
top_p 0.95, captured graphs.

For each model a fixed batch (default 64 images) and n in {1, 4, 16, 64}: the shared call and the plain repeated-cond call of the same build,
alternated in one process, one warm-up each, device events, medians of 5 with the spread (max - min) of the repeats as the noise margin.
Two model objects with the same weights, one per form: a handle's KV workspace has one layout at a time, so alternating the forms on one
handle would re-lay it and recapture its graphs at every call.

Columns: images/s; prefill ms = a call in which every code is kept (keep_mask all true: inputs, text prefill and the copy back, no position);
decode-attention us per launch of the body stack and the head stack together (the engine's event bracket, rqamd_rqt_set_profile(1): eager
launches) ; rqamd_rqt_kv_bytes.

Optional arguments: the batch (default 64), then model names (txt3900m, cc3m)."""
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
MODELS = {'txt3900m': 'RQT_TXT_3900M', 'cc3m': 'RQT_CC3M_654M'}
FANS = (1, 4, 16, 64)


class Aux:
    def __init__(self, V, depth):
        t = torch.randn((V, 256), device=dev)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def time_ms(fns, reps=REPS):
    """fns: name -> callable; one warm-up each, then alternated; returns name -> (median, min, max) ms per call"""
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
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in res.items()}


def attn_us(ar, fn):
    """decode-attention microseconds per launch of one call, from the engine's event bracket (eager launches)"""
    eng = ar._eng()
    eng.set_profile(1)
    try:
        fn()
        torch.cuda.synchronize()
        p = eng.get_profile()
    finally:
        eng.set_profile(0)
    return 1e3 * p['attn_ms_total'] / max(p['attn_launches'], 1), p['attn_launches']


def main(batch, names):
    print(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_attn_shared.hip', 'rqt_kernels.hip', 'engine_rqt.hip'))}")
    lost = []
    for name in names:
        cfg = getattr(cfgs, MODELS[name])
        models = []
        for _ in range(2):
            torch.manual_seed(0)
            with torch.device(dev):
                models.append(RQTransformer(cfg).eval())
        shared, plain = models
        aux = Aux(16384, 4)
        (H, W, D) = cfg['block_size']
        P = cfg['block_size_cond'] - 1
        part = torch.randint(0, 16384, (batch, H, W, D), device=dev)
        keep_all = torch.ones((H, W), dtype=torch.bool, device=dev)
        print(f'== {name}: {batch} images, {P} text tokens + {H} x {W} x {D} codes, top_k 1024 / top_p 0.95, graphs, medians of {REPS} (noise = max - min of the repeats)')
        print('    n  groups |  images/s shared (noise)   plain (noise)   ratio | prefill ms shared  plain | attn us/launch shared  plain | KV MiB shared  plain')
        for fan in reversed(FANS):                     # (fewest groups first: the group workspace only ever grows, and its size is a column)
            if batch % fan:
                continue
            G = batch // fan
            cond = torch.randint(0, 16384, (G, P + 1), device=dev)
            full = cond.repeat_interleave(fan, 0).contiguous()

            def run_shared(**kw):
                with shared.shared_cond(fan):
                    return shared.sample(part, aux, cond=cond, **KW, **kw)

            def run_plain(**kw):
                return plain.sample(part, aux, cond=full, **KW, **kw)
            t = time_ms({'shared': run_shared, 'plain': run_plain})
            pf = time_ms({'shared': lambda: run_shared(keep_mask=keep_all), 'plain': lambda: run_plain(keep_mask=keep_all)})
            a_s, n_s = attn_us(shared, run_shared)
            a_p, n_p = attn_us(plain, run_plain)
            assert n_s == n_p, (n_s, n_p)
            run_shared()
            run_plain()                                    # (the workspaces as the last full calls left them)
            kv_s, kv_p = shared._eng().kv_bytes(), plain._eng().kv_bytes()
            (ms, lo_s, hi_s), (mp, lo_p, hi_p) = t['shared'], t['plain']
            ips_s, ips_p = 1e3 * batch / ms, 1e3 * batch / mp
            noise_s, noise_p = ips_s * (hi_s - lo_s) / ms, ips_p * (hi_p - lo_p) / mp
            print(f'  {fan:3d}  {G:6d} | {ips_s:9.1f} ({noise_s:6.1f})  {ips_p:9.1f} ({noise_p:6.1f})  {ips_s / ips_p:6.3f} | {pf["shared"][0]:10.2f}  {pf["plain"][0]:9.2f} |'
                  f' {a_s:12.2f}  {a_p:9.2f} | {kv_s / 2 ** 20:9.1f}  {kv_p / 2 ** 20:9.1f}')
            if fan >= 2 and ips_s + max(noise_s, noise_p) < ips_p:
                lost.append((name, fan, ips_s / ips_p))
        del shared, plain, models
        torch.cuda.empty_cache()
    print('== shared loses beyond the noise at n >= 2: ' + (', '.join(f'{n} n={f} ({r:.3f} x)' for n, f, r in lost) if lost else 'nowhere in this run'))


if __name__ == '__main__':
    args = sys.argv[1:]
    batch = int(args[0]) if args and args[0].isdigit() else 64
    names = [a for a in args if a in MODELS] or list(MODELS)
    main(batch, names)
