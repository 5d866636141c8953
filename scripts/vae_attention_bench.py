#!/usr/bin/env python
"""AttnBlock attention beyond 64 tokens: the tiled MFMA kernel against the wavefront-per-query kernel -> profiles/vae_attention_bench.txt

    python scripts/vae_attention_bench.py [--part kernel|e2e|all] [--rounds R]

1. kernel: rqamd_dbg_vae_attn forms 1 (wavefront per query) and 3 (tiled) at (128 images, 256 tokens, C 512) -- one FFHQ attention of a
   128-image chunk -- and (16, 1024, 512); form 3 alone at (4, 4096, 128), which form 1 refuses.  Both forms are warmed up, then timed
   alternately (A B A B ...) with device events over windows of >= ~0.2 s of launches; median and [min, max] over the rounds, and the
   rate over the algorithm's 4 T^2 C FLOP per image.
2. e2e: the released FFHQ RQ-VAE shape (attn_resolutions [16]: five 256-token attentions at C 512, three in the decoder and two in the
   encoder), synthetic weights: ms per image of decode_code and of get_codes at 128 images, with and without RQAMD_VAE_ATTN_VALU.  The
   switch is read once per process, so every measurement is a fresh child; the two settings alternate (A B A B).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'rq-vae-transformer_amd'))

import torch  # noqa: E402

from rqvae import _native  # noqa: E402

DEV = 'cuda:0'


def _time_window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


def _fmt(ts):
    return '%8.3f ms  [%.3f, %.3f]' % (statistics.median(ts), min(ts), max(ts))


def part_kernel(rounds):
    print('== kernel A/B through rqamd_dbg_vae_attn (ms per launch: median [min, max] over %d alternating rounds)' % rounds)
    for B, T, C, forms in ((128, 256, 512, (1, 3)), (16, 1024, 512, (1, 3)), (4, 4096, 128, (3,))):
        g = torch.Generator(device=DEV).manual_seed(T + C)
        qkv = torch.randn((B, T, 3 * C), generator=g, device=DEV).bfloat16()
        outs = {f: torch.empty((B, T, C), dtype=torch.bfloat16, device=DEV) for f in forms}
        run = {f: (lambda f=f: _native.dbg_vae_attn(qkv, form=f, out=outs[f])) for f in forms}
        n = {}
        for f in forms:                      # warm-up, and a launch count that fills ~0.2 s
            run[f]()
            torch.cuda.synchronize()
            t = _time_window(run[f], 3)
            n[f] = max(3, min(2000, int(200.0 / max(t, 1e-3))))
        ts = {f: [] for f in forms}
        for _ in range(rounds):
            for f in forms:
                ts[f].append(_time_window(run[f], n[f]))
        flop = 4.0 * T * T * C * B
        for f in forms:
            med = statistics.median(ts[f])
            print('  (%4d images, %4d tokens, C %3d) form %d %-19s %s   %7.2f TFLOP/s  (%d launches per window)'
                  % (B, T, C, f, '(wavefront/query)' if f == 1 else '(tiled MFMA)', _fmt(ts[f]), flop / (med * 1e-3) / 1e12, n[f]))
        if len(forms) == 2:
            d = (outs[1].float() - outs[3].float()).abs()
            print('      speed-up of the tiled kernel %.1fx; outputs differ by at most %.3e (mean %.3e; bf16 outputs of magnitude <= %.2f)'
                  % (statistics.median(ts[1]) / statistics.median(ts[3]), float(d.max()), float(d.mean()), float(outs[1].float().abs().max())))


def child_e2e(what, images, reps):
    """one process: ms per image of decode_code / get_codes of the FFHQ RQ-VAE shape at `images` images"""
    import copy
    from rqvae import presets
    from rqvae.models import create_model
    from rqvae.utils.config import Config, augment_arch_defaults
    torch.manual_seed(0)
    vae, _ = create_model(augment_arch_defaults(Config(copy.deepcopy(presets.RQVAE['ffhq']))))
    vae = vae.to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(1)
    if what == 'decode_code':
        arg = torch.randint(0, 2048, (images, 8, 8, 4), generator=g, device=DEV)
        fn = lambda: vae.decode_code(arg)
    else:
        arg = torch.randn((images, 3, 256, 256), generator=g, device=DEV).clamp_(-1, 1)
        fn = lambda: vae.get_codes(arg)
    with torch.no_grad():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / images)
    print('RESULT ' + json.dumps(ts))


def part_e2e(rounds, images, reps):
    print('== FFHQ RQ-VAE shape, %d images per call, ms per image (median [min, max] over %d processes x %d calls, settings alternating)'
          % (images, rounds, reps))
    for what in ('decode_code', 'get_codes'):
        ts = {'tiled': [], 'RQAMD_VAE_ATTN_VALU': []}
        for _ in range(rounds):
            for tag in ts:
                env = dict(os.environ)
                env.pop('RQAMD_VAE_ATTN_VALU', None)
                if tag != 'tiled':
                    env['RQAMD_VAE_ATTN_VALU'] = '1'
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', what, '--images', str(images), '--reps', str(reps)],
                                   env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                ts[tag] += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        for tag in ts:
            print('  %-12s %-20s %s' % (what, tag, _fmt(ts[tag])))
        print('      %s: %.3f ms per image saved by the tiled kernel (%.1f %%)'
              % (what, statistics.median(ts['RQAMD_VAE_ATTN_VALU']) - statistics.median(ts['tiled']),
                 100.0 * (1.0 - statistics.median(ts['tiled']) / statistics.median(ts['RQAMD_VAE_ATTN_VALU']))))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['kernel', 'e2e', 'all'])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--e2e-rounds', type=int, default=2)
    ap.add_argument('--images', type=int, default=128)
    ap.add_argument('--reps', type=int, default=4)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('vae_attention_bench: needs an MI355X (no CPU path)')
    if a.child:
        child_e2e(a.child, a.images, a.reps)
        sys.exit(0)
    print('vae_attention_bench on %s, kernels %s' % (torch.cuda.get_device_name(0), _native.kernel_source_hash(('vae_kernels.hip', 'rq_hip.h'))))
    if a.part in ('kernel', 'all'):
        part_kernel(a.rounds)
    if a.part in ('e2e', 'all'):
        part_e2e(a.e2e_rounds, a.images, a.reps)
