"""Strict elementwise checks of the bf16 GEMM / conv kernels against an fp64 reference (used by tests/test_gpu_gemm_conv.py; the
evidence that these checks can fail is tests/test_kernel_check.py).

Reference: fp64 from the bf16-rounded operands, ref = A W^T + bias, and the magnitude S = |A| |W|^T + |bias| (+ |resid|) of the same
sum.  A kernel that adds n terms in fp32 one after another (K / 16 MFMA steps, the K splits, the epilogue additions) is off by at
most ~n 2^-24 S; the checks allow

    fp32 outputs:   |out - ref| <= c 2^-24 n S                                  elementwise
    bf16 outputs:   the same + half a bf16 ulp of the value (round to nearest even; truncation is off by up to a whole ulp)
    GELU:           the pre-activation bound times max |gelu'| = 1.13, + the erf polynomial's own error (gemm.h: rq_gelu_erf)

with c chosen per kernel family at 2-4 x the largest err / (2^-24 n S) measured on MI355X (printed under -s).  Outputs are views into
NaN-filled buffers (nothing outside the written region may change) and the operands sit in NaN-poisoned buffers with extra rows past
M and N (a read past the end that reaches a stored value shows up as NaN)."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24                 # fp32 unit roundoff
MFMA_K = 16                    # K depth of one v_mfma_f32_32x32x16_bf16: one fp32 accumulation step
GELU_SLOPE = 1.13              # max |d/dx x Phi(x)| = 1.1289
GUARD = 4096                   # guard elements on either side of an output

# c per kernel family: 2-4 x the largest err / (2^-24 n S) measured on MI355X (tests/test_gpu_gemm_conv.py prints the observed values)
# (maxima on MI355X, all families x epilogues x edges of that file: skinny 0.016, stream 0.088, reg 0.117, lds 0.182, mid 0.130,
# p8 0.117, rb 0.236, conv 0.015, halo 0.027, conv_in 0.239, conv_out 0.029)
C = {'skinny': 0.05, 'stream': 0.25, 'reg': 0.35, 'lds': 0.5, 'mid': 0.4, 'rb': 0.6, 'p8': 0.35, 'conv': 0.05, 'halo': 0.06,
     'conv_in': 0.7, 'conv_out': 0.09}
# largest observed err / (2^-24 n S) per family (filled by the checks, printed by the GPU tests)
OBSERVED = {}


def steps(K, splits=1, epi_adds=1):
    """n: sequential fp32 accumulation steps behind one output"""
    return K // MFMA_K + splits + epi_adds


def bf16_ulp(x):
    """ulp of bf16 at |x| (fp64 tensor), from the exponent: 2^(e - 7) for |x| in [2^e, 2^(e+1)); 2^-133 below the normal range"""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, -133, e.to(torch.int32) - 8)                  # (frexp(0) has exponent 0)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e.clamp(min=-133))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_err(x):
    """error of the kernel's GELU before its bf16 rounding: the erf polynomial (< 2.3e-5, times |x| / 2) + its fp32 arithmetic"""
    return 5e-5 + 1.2e-5 * x.abs()


def round_bf16_trunc(x):
    """bf16 by dropping the low 16 bits of the fp32 value (what a kernel that forgot to round would store)"""
    b = x.float().contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ references
def gemm_ref(a, w, bias=None, k0=0, k1=None):
    """fp64 a[:, k0:k1] w[:, k0:k1]^T (+ bias) and S = |a| |w|^T (+ |bias|) over the same K range"""
    a64, w64 = a[:, k0:k1].double(), w[:, k0:k1].double()
    ref, S = a64 @ w64.T, a64.abs() @ w64.abs().T
    if bias is not None:
        b = bias.double()
        ref += b
        S += b.abs()
    return ref, S


def im2col64(x, ksize, stride=1, ups=0):
    """x NHWC (B, Hs, Ws, C) -> fp64 (B, C k k, Ho Wo) columns of the conv the engine runs: nearest 2x upsample when ups, the
    reference's F.pad (0, 1, 0, 1) before a stride-2 conv (layers.py:50-54), padding k // 2 otherwise"""
    xi = x.double().permute(0, 3, 1, 2)
    if ups:
        xi = xi.repeat_interleave(2, 2).repeat_interleave(2, 3)
    xi = F.pad(xi, (0, 1, 0, 1) if stride == 2 else (ksize // 2,) * 4)
    return F.unfold(xi, ksize, stride=stride)


def conv_ref(x, w, bias=None, resid=None, stride=1, ups=0, xulp=None):
    """fp64 conv of NHWC x with w (Cout, k, k, Cin) as an (M = B Ho Wo, Cout) matrix, its S, and (xulp given: a per-element
    uncertainty of the input, e.g. one bf16 ulp of a normalised input) the bound |W| * xulp that it propagates to, else None"""
    Cout, k, _, Cin = w.shape
    w2 = w.double().permute(0, 3, 1, 2).reshape(Cout, Cin * k * k)
    cols = im2col64(x, k, stride, ups)
    ref = (w2 @ cols).permute(0, 2, 1).reshape(-1, Cout)
    S = (w2.abs() @ cols.abs()).permute(0, 2, 1).reshape(-1, Cout)
    del cols
    extra = None
    if xulp is not None:
        extra = (w2.abs() @ im2col64(xulp, k, stride, ups)).permute(0, 2, 1).reshape(-1, Cout)
    if bias is not None:
        ref += bias.double()
        S += bias.double().abs()
    if resid is not None:
        r = resid.double().reshape(-1, Cout)
        ref += r
        S += r.abs()
    return ref, S, extra


def subpixel_taps64(w):
    """fp64 pre-summed taps of nearest 2x upsample + 3x3 conv (w (Cout, 3, 3, Cin)) as four 2 x 2 convs over the source image:
    (4, Cout, 2, 2, Cin), class (py, px) = 2 py + px, tap (a, b) = the 3 x 3 taps that read source pixel (y + py - 1 + a, x + px - 1 + b)"""
    sets = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    w64 = w.double()
    out = torch.zeros((4, w.shape[0], 2, 2, w.shape[3]), dtype=torch.float64, device=w.device)
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    for ky in sets[py][a]:
                        for kx in sets[px][b]:
                            out[2 * py + px, :, a, b] += w64[:, ky, kx]
    return out


def subpixel_conv_ref(xs, wsub, bias=None):
    """fp64 sub-pixel form of the upsample conv with the given pre-summed taps wsub (4, Cout, 2, 2, Cin): output pixel (2 y + py, 2 x + px)
    is a 2 x 2 conv over the zero-padded source image xs (B, Hs, Ws, Cin); returns ((B 2Hs 2Ws, Cout) ref, S)"""
    B, Hs, Ws, Cin = xs.shape
    Cout = wsub.shape[1]
    xp = F.pad(xs.double().permute(0, 3, 1, 2), (1, 1, 1, 1))
    ref = torch.empty((B, Hs, 2, Ws, 2, Cout), dtype=torch.float64, device=xs.device)
    S = torch.empty_like(ref)
    for py in (0, 1):
        for px in (0, 1):
            cols = F.unfold(xp[:, :, py:py + Hs + 1, px:px + Ws + 1], 2)
            w2 = wsub[2 * py + px].double().permute(0, 3, 1, 2).reshape(Cout, Cin * 4)
            ref[:, :, py, :, px] = (w2 @ cols).permute(0, 2, 1).reshape(B, Hs, Ws, Cout)
            S[:, :, py, :, px] = (w2.abs() @ cols.abs()).permute(0, 2, 1).reshape(B, Hs, Ws, Cout)
            del cols
    ref, S = ref.reshape(-1, Cout), S.reshape(-1, Cout)
    if bias is not None:
        ref += bias.double()
        S += bias.double().abs()
    return ref, S


# ------------------------------------------------------------------------------------------------ buffers
def poisoned(t, extra_rows=67):
    """t (rows, ...) copied into the front of a NaN-filled buffer with extra_rows more rows; returns the contiguous front view"""
    buf = torch.full((t.shape[0] + extra_rows,) + tuple(t.shape[1:]), float('nan'), dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def guarded(shape, dtype, device):
    """a NaN-filled output of `shape` inside a NaN-filled flat buffer with GUARD elements on either side: (buf, view)"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def check_guard(buf, n, what=''):
    """everything of buf outside [GUARD, GUARD + n) is still NaN"""
    for part, name in ((buf[:GUARD], 'before'), (buf[GUARD + n:], 'after')):
        bad = ~torch.isnan(part.float())
        if bool(bad.any()):
            raise AssertionError(f'{what}: {int(bad.sum())} stores {name} the output (first at guard offset {int(bad.nonzero()[0, 0])})')


def check_nan(t, what=''):
    """t (slabs the kernel must not write) is still all NaN"""
    bad = ~torch.isnan(t.float())
    if bool(bad.any()):
        raise AssertionError(f'{what}: {int(bad.sum())} stores into a region that must stay unwritten')


# ------------------------------------------------------------------------------------------------ checks
def _report(out, want, err, bound, what):
    bad = ~(err <= bound)                          # NaN counts as bad
    if bool(bad.any()):
        t = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {t}: out {float(out[t])!r}, '
                             f'ref {float(want[t])!r}, |err| {float(err[t]):.3e} > bound {float(bound[t]):.3e}')


def _note(family, ratio):
    if family is not None and ratio == ratio:
        OBSERVED[family] = max(OBSERVED.get(family, 0.0), ratio)
    return ratio


def check_f32(out, ref, S, n, c, extra=None, what='', family=None):
    """fp32 output: |out - ref| <= c 2^-24 n S (+ extra: input uncertainty, already a bound) elementwise.  Returns the observed max
    (err - extra) / (2^-24 n S)."""
    unit = (U * n) * S
    slack = extra if extra is not None else 0.0
    err = (out.double() - ref).abs()
    ratio = float(((err - slack).clamp_min(0.0) / unit.clamp_min(1e-300)).max())
    _report(out, ref, err, c * unit + slack, what)
    return _note(family, ratio)


def check_bf16(out, ref, S, n, c, gelu=False, extra=None, what='', family=None):
    """bf16 output of the fp32 value ref +- (c 2^-24 n S + extra), optionally through GELU, rounded to nearest even: the bound adds half
    a bf16 ulp (of the largest admissible magnitude, so that a value that rounds across a power of two is judged by the ulp it lands
    on).  Returns the observed max (err - half an ulp - extra) / (2^-24 n S)."""
    unit = (U * n) * S
    slack = extra if extra is not None else 0.0
    pre = c * unit + slack
    want = ref
    if gelu:
        want = gelu64(ref)
        pre = GELU_SLOPE * pre + gelu_err(ref)
        slack = GELU_SLOPE * slack + gelu_err(ref)
        unit = GELU_SLOPE * unit
    err = (out.double() - want).abs()
    excess = (err - 0.5 * bf16_ulp(want) - slack).clamp_min(0.0)
    ratio = float((excess / unit.clamp_min(1e-300)).max())
    _report(out, want, err, pre + 0.5 * bf16_ulp(want.abs() + pre), what)
    return _note(family, ratio)
