#!/usr/bin/env python
"""Long-context measurements (body contexts beyond 256 tokens) at the 1.4B widths: E 1536, 24 heads, two body layers + one head layer
(oracle.configs.RQT_WIDE with block_size (32, 32, 4)).  Device events, warm-up, the variants of a group alternated in one process.

1. decode attention alone (rq_launch_attn_decode called directly on scratch buffers): the chunked kernel at t = 300 and 1023 (Tcap 1088),
   64 and 512 rows, against the yardstick -- the 32-block register kernel at t = 255, Tcap 256 -- in microseconds and bytes/s of K + V read
   (data sheet: 8 TB/s); at 64 rows both forms of the chunked kernel (one / four wavefronts per pair, RQAMD_ATTN_LONG_SPLIT).
2. one-pass forward at context 1087 (32 x 32 x 4 behind 64 text tokens), 8 images: time, and the tiled attention kernel's share (the same
   launch timed alone, times the number of body layers).
3. sample() at 64 rows: ms per position below 256 tokens (a 16 x 16 map) and above (the 768 further positions of a 32 x 32 map).

The two launchers are C++ functions of librqamd.so, not part of its C ABI: this script finds them by their mangled names."""
import ctypes as C
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
lib = _native.lib()
E, NH = 1536, 24
PEAK = 8e12


class AttnDecodeArgs(C.Structure):
    _fields_ = [('qkv', C.c_void_p), ('kc', C.c_void_p), ('vc', C.c_void_p), ('ksc', C.c_void_p), ('vsc', C.c_void_p), ('y', C.c_void_p),
                ('step', C.c_void_p), ('step_off', C.c_int), ('t_max', C.c_int), ('rows', C.c_int), ('nh', C.c_int), ('E', C.c_int), ('Tcap', C.c_int)]


class AttnPrefillArgs(C.Structure):
    _fields_ = [('qkv', C.c_void_p), ('kc', C.c_void_p), ('vc', C.c_void_p), ('ksc', C.c_void_p), ('vsc', C.c_void_p), ('y', C.c_void_p),
                ('n_img', C.c_int), ('P', C.c_int), ('nh', C.c_int), ('E', C.c_int), ('Tcap', C.c_int)]


launch_decode = getattr(lib, '_Z21rq_launch_attn_decodeRK14AttnDecodeArgsP12ihipStream_t')
launch_prefill = getattr(lib, '_Z22rq_launch_attn_prefillRK15AttnPrefillArgsP12ihipStream_t')
for fn in (launch_decode, launch_prefill):
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]


def time_us(fns, reps=20, inner=10):
    """fns: name -> callable; alternated, `inner` launches between two events; returns name -> (median, min) microseconds per launch"""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in res.items()}


def decode_case(rows, Tcap, t, split=None):
    qkv = torch.randn((rows, 3 * E), device=dev).to(torch.bfloat16)
    kc = torch.randn((rows * NH * Tcap * 64,), device=dev, dtype=torch.bfloat16)
    vc = torch.randn((rows * NH * Tcap * 64,), device=dev, dtype=torch.bfloat16)
    y = torch.empty((rows, E), device=dev, dtype=torch.bfloat16)
    a = AttnDecodeArgs(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), None, None, y.data_ptr(), None, t, Tcap - 1 if Tcap > 256 else t, rows, NH, E, Tcap)
    keep = (qkv, kc, vc, y)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        if split is not None:
            os.environ['RQAMD_ATTN_LONG_SPLIT'] = split
        rc = launch_decode(C.byref(a), stream)
        os.environ.pop('RQAMD_ATTN_LONG_SPLIT', None)
        assert rc == 0, rc
        return keep
    return run, rows * NH * (t + 1) * 64 * 2 * 2


def section_decode():
    print('== 1. decode attention alone (E 1536, 24 heads; K + V bytes read / time; data sheet 8 TB/s)')
    for rows in (64, 512):
        cases = {'yardstick: 32-block register kernel, Tcap 256, t=255': decode_case(rows, 256, 255)}
        for t in (300, 1023):
            if rows == 64:
                cases[f'chunked, 1 wavefront / pair, t={t}'] = decode_case(rows, 1088, t, '0')
                cases[f'chunked, 4 wavefronts / pair, t={t}'] = decode_case(rows, 1088, t, '1')
            else:
                cases[f'chunked (default form), t={t}'] = decode_case(rows, 1088, t)
        out = time_us({k: v[0] for k, v in cases.items()})
        for k, (med, lo) in out.items():
            by = cases[k][1]
            print(f'  rows {rows:4d}  {k:56s} {med:8.1f} us (min {lo:7.1f})  {by / 1e6:8.1f} MB  {by / med / 1e6:6.2f} TB/s = {by / med * 1e6 / PEAK * 100:5.1f} % of 8 TB/s')
        del cases
        torch.cuda.empty_cache()


class Aux:
    def __init__(self, V, depth):
        t = torch.randn((V, 256), device=dev)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def wide(block_size, block_cond):
    cfg = cfgs.rqt(1536, 24, 2, 1, 16384, vocab_cond=1000, block_cond=block_cond, block_size=block_size)
    torch.manual_seed(0)
    return RQTransformer(cfg).to(dev).eval(), cfg


def section_onepass():
    print('== 2. one-pass forward, context 1087 (32 x 32 x 4 behind 64 text tokens), 8 images, 2 body + 1 head layers')
    ar, cfg = wide((32, 32, 4), 64)
    aux = Aux(16384, 4)
    codes = torch.randint(0, 16384, (8, 32, 32, 4), device=dev)
    cond = torch.randint(0, 1000, (8, 64), device=dev)
    n_img, P = 3, 1087                      # fwd.chunk_rows = 4096: three images per body chunk
    qkv = torch.randn((n_img * P, 3 * E), device=dev).to(torch.bfloat16)
    y = torch.empty((n_img * P, E), device=dev, dtype=torch.bfloat16)
    a = AttnPrefillArgs(qkv.data_ptr(), None, None, None, None, y.data_ptr(), n_img, P, NH, E, P)
    stream = torch.cuda.current_stream().cuda_stream
    out = time_us({'log_probs (one pass)': lambda: ar.log_probs(codes, aux, cond=cond),
                   'tiled attention, 3 images, one layer': lambda: launch_prefill(C.byref(a), stream)}, reps=8, inner=2)
    tot, att = out['log_probs (one pass)'][0], out['tiled attention, 3 images, one layer'][0]
    for k, (med, lo) in out.items():
        print(f'  {k:40s} {med / 1e3:9.3f} ms (min {lo / 1e3:9.3f})')
    share = att * (8 / 3) * 2 / tot
    flops = 4.0 * 64 * P * (P + 1) / 2 * NH * n_img
    print(f'  tiled attention share of the pass: 2 layers x 8/3 chunks x {att / 1e3:.3f} ms = {share * 100:.1f} % ({flops / att / 1e6:.2f} TFLOP/s causal, VALU fp32)')
    del ar
    torch.cuda.empty_cache()


def section_sample():
    print('== 3. sample(), 64 rows, graphs: ms per position below / above 256 tokens')
    times = {}
    for bs in ((16, 16, 4), (32, 32, 4)):
        ar, cfg = wide(bs, 1)
        aux = Aux(16384, 4)
        part = torch.zeros((64,) + bs, device=dev, dtype=torch.long)
        cond = torch.zeros((64, 1), device=dev, dtype=torch.long)
        out = time_us({'s': lambda: ar.sample(part, aux, cond=cond, top_k=1024, top_p=0.95)}, reps=3, inner=1)
        times[bs] = out['s'][0] / 1e3
        print(f'  block_size {bs}: {times[bs]:9.2f} ms per batch')
        del ar
        torch.cuda.empty_cache()
    below = times[(16, 16, 4)] / 256
    above = (times[(32, 32, 4)] - times[(16, 16, 4)]) / 768
    print(f'  per position: {below:.4f} ms below 256 tokens, {above:.4f} ms above (positions 256 .. 1023 of the 32 x 32 map)')


if __name__ == '__main__':
    which = sys.argv[1:] or ['decode', 'onepass', 'sample']
    print(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'rq_hip.h'))}")
    for w in which:
        {'decode': section_decode, 'onepass': section_onepass, 'sample': section_sample}[w]()
