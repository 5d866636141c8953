#!/usr/bin/env python
"""Min-p and locally typical sampling: what the two stages cost (rqamd_sample_logits_trunc, RQTransformer.sample(min_p=, typical_p=)).

Part 1, the sampler alone: us per stand-alone call over 4096 x 16384 fp32 logits (N(0, 2.5)), the same inputs for every configuration,
device events, one warm-up each, configurations alternated in one process, medians and minima of `reps` rounds:

  (p) the parent commit's library, rqamd_sample_logits at k = 1024 / p = 0.95   (only with --parent-lib PATH: a librqamd.so built from
      the parent commit)
  (a) this commit, the same call through rqamd_sample_logits_trunc with both filters off   (the same kernel: must be level with (p))
  (b) k = 1024 + min-p 0.05
  (c) k = 1024 + typical 0.95
  (d) k = 1024 / p = 0.95 + min-p 0.05 + typical 0.95
  (e) typical 0.95 alone, no top-k: the general (LDS) form

Expected: min-p adds one block maximum, one pass and one sum; typical one logf pass, one reduction and a 31-step search, what top-p
costs: (c) within about 1.3 x (p), (d) within 2 x.  Nothing is asserted about the times.

Part 2, the engine: one sample() of the 1.4B shape (oracle.configs.RQT_IN_1400M, random weights, 8 x 8 x 4 codes, vocabulary 16384,
captured graphs) at 64 images, top_k = 1024 / top_p = 0.95, with and without typical_p = 0.95.  Skipped with --no-engine.

The output is also written to profiles/trunc_sampling_bench.txt."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'rq-vae-transformer_amd'))
import torch  # noqa: E402
from rqvae import _native  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device('cuda', 0)
ROWS, V, TOP_K, TOP_P, MIN_P, TYP = 4096, 16384, 1024, 0.95, 0.05, 0.95
OUT = os.path.join(ROOT, 'profiles', 'trunc_sampling_bench.txt')
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


def time_all(fns, reps, inner=1):
    """fns: name -> callable; one warm-up each, then alternated; returns name -> (median, min) ms per call"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            res[k].append(timed(lambda: [f() for _ in range(inner)]) / inner)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in res.items()}


def sampler_part(parent_lib, reps=15):
    torch.manual_seed(0)
    logits = 2.5 * torch.randn((ROWS, V), device=dev)
    out = torch.empty((ROWS,), dtype=torch.int64, device=dev)
    flags = torch.empty((ROWS,), dtype=torch.int32, device=dev)
    p, st = _native.ptr, _native.stream_of(logits)
    lib = _native.lib()

    def trunc(k, tp, mp, ty):
        def f():
            _native.check(lib.rqamd_sample_logits_trunc(p(logits), None, ROWS, V, 1.0, k, tp, mp, ty, 1.0, None, None, None, None, None, None, None,
                                                        7, 5, p(out), None, None, p(flags), st))
        return f
    fns = {}
    if parent_lib:
        old = C.CDLL(parent_lib)
        old.rqamd_sample_logits.restype = C.c_int
        old.rqamd_sample_logits.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4

        def parent():
            assert old.rqamd_sample_logits(p(logits), ROWS, V, 1.0, TOP_K, TOP_P, 7, 5, p(out), None, p(flags), st) == 0
        fns['(p) parent, k / p'] = parent
    fns['(a) k / p, filters off'] = trunc(TOP_K, TOP_P, 0.0, -1.0)
    fns['(b) k + min-p'] = trunc(TOP_K, -1.0, MIN_P, -1.0)
    fns['(c) k + typical'] = trunc(TOP_K, -1.0, 0.0, TYP)
    fns['(d) k / p + min-p + typical'] = trunc(TOP_K, TOP_P, MIN_P, TYP)
    fns['(e) typical, no top-k'] = trunc(0, -1.0, 0.0, TYP)
    if parent_lib:                                          # the same draws from both libraries before anything is timed
        fns['(p) parent, k / p']()
        a = out.clone()
        fns['(a) k / p, filters off']()
        say(f'(a) draws what (p) draws: {bool(torch.equal(a, out))}')
    res = time_all(fns, reps, inner=4)
    base = res.get('(p) parent, k / p', res['(a) k / p, filters off'])
    say(f'== sampler alone, {ROWS} x {V}, k = {TOP_K}, p = {TOP_P}, min_p = {MIN_P}, typical_p = {TYP}; us per call, medians of {reps} (minima)')
    for k, (med, lo) in res.items():
        say(f'  {k:30s} {1e3 * med:9.1f} us (min {1e3 * lo:9.1f})   {med / base[0]:5.2f} x {"(p)" if parent_lib else "(a)"}')


class Aux:
    def __init__(self, V, depth):
        t = torch.randn((V, 256), device=dev)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def engine_part(B=64, reps=5):
    from oracle import configs as cfgs
    from rqvae.models.rqtransformer import RQTransformer
    cfg = cfgs.RQT_IN_1400M
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    aux = Aux(V, 4)
    (H, W, D) = cfg['block_size']
    part = torch.zeros((B, H, W, D), dtype=torch.long, device=dev)
    cond = torch.randint(0, max(cfg['vocab_size_cond'], 1), (B, 1), device=dev)
    fns = {'(a) top_k / top_p': lambda: ar.sample(part, aux, cond=cond, top_k=TOP_K, top_p=TOP_P),
           '(b) + typical_p': lambda: ar.sample(part, aux, cond=cond, top_k=TOP_K, top_p=TOP_P, typical_p=TYP)}
    res = time_all(fns, reps)
    (ta, tb) = res.values()
    say(f'== sample(), 1.4B shape, B = {B}, {H} x {W} x {D}, top_k {TOP_K} / top_p {TOP_P}, graphs, medians of {reps} (minima)')
    for k, (med, lo) in res.items():
        say(f'  {k:20s} {med:9.2f} ms per call (min {lo:9.2f})')
    say(f'  (b) - (a): {tb[0] - ta[0]:+.2f} ms = {100 * (tb[0] / ta[0] - 1):+.2f} % (medians)')


if __name__ == '__main__':
    args = sys.argv[1:]
    parent = args[args.index('--parent-lib') + 1] if '--parent-lib' in args else None
    say(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'engine_rqt.hip'))}")
    sampler_part(parent)
    if '--no-engine' not in args:
        engine_part()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as fh:
        fh.write('scripts/trunc_sampling_bench.py\n' + '\n'.join(lines) + '\n')
