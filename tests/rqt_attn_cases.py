"""Shared by tests/test_emu_rqt_attention.py and tests/test_gpu_rqt_attention.py: seeded inputs, the fp64 reference, the elementwise bound,
the side-effect checks and the case lists of the stand-alone checks of the RQ-Transformer's attention kernels (csrc/rqt_kernels.hip) through
rqamd_dbg_rqt_attn_decode / _prefill / _packed.

Reference: fp64 from the 16-bit-rounded operands, ref = softmax(q . k_j / sqrt(hd), j <= t) v and A = sum_j p_j |v_j|, the magnitude of the
same sum.  A cached key / value of the 8-bit formats is (byte - 128) * scale exactly as AttnDecodeArgs defines it; this token's own k / v is
always bf16.  Bound, elementwise:

    |out - ref| <= 1/2 ulp_bf16(ref) + c 2^-20 A      (+ UNDERFLOW = 1.6e-33, fp32's underflow threshold over all keys: see below)

The first term is the one rounding of the output.  The second is the fp32 work before it: a 64-term fp32 dot product behind every score, the
rounding of (s - m) log2(e) (its relative effect on a weight grows with |s - m|: the 'peaked' inputs), the one-instruction exp2, the fp32
weighted sum, and for the 8-bit keys the cancellation in (sum q byte - 128 sum q) scale.  c is measured on MI355X against this reference;
one constant per cache class, 3 x the largest value observed over all cases of the class (the convention of C_BOUND in vae_attn_cases.py):

    bf16 caches: C_BF16 = 6.84 = 3 x 2.279, observed on the generic decode kernel at head size 256 (a 256-term sequential dot product);
                 the chunked kernel reaches 1.981 on the 'low' inputs (scores near -128: the rounding of (s - m) log2(e) at its
                 largest), every 64-wide register / prefill / packed kernel stays below 0.07
    8-bit caches: C_INT8 = 0.19 = 3 x 0.062, observed on the small kernel with int8kv
    (OBSERVED_MI355X below lists the per-class maxima; most classes sit at 0.000: half an output ulp covers the whole error)

The bf16-cache classes must stay at or below c = 8 (2^-17 A, the unit of the VAE's tiled kernel, which carries bf16 hi + lo probabilities;
these kernels keep fp32 weights).  The emulator's exp2f is the host's, so its observed values sit below the GPU's; the bound is the same.

Buffers: qkv, both caches, both scale arrays and y live inside larger buffers with poisoned guards on both sides; cache rows >= t hold
NaN (bf16 rows, scales) or a fixed byte pattern, y starts as NaN.  A stray read becomes a NaN in the output, a stray write is seen; neither
becomes a fault.  No case passes arguments that reach a kernel trap: t <= t_max < Tcap everywhere, and the refusals are host-side."""
import math

import torch

from kernel_check import GUARD, bf16_ulp, check_guard, guarded

# largest observed c on MI355X per kernel class / cache format (every class not listed: 0.000, the output rounding alone)
OBSERVED_MI355X = {'generic/bf16': 2.279, 'long4/bf16': 1.981, 'long1/bf16': 1.981, 'packed-hd64/bf16': 0.065, 'packed-vec/bf16': 0.048,
                   'packed-scalar/bf16': 0.046, 'plain/bf16': 0.064, 'tiled/bf16': 0.062, 'reg3/bf16': 0.062, 'reg3x2/bf16': 0.014,
                   'reg8/bf16': 0.010, 'chain-dyn16/bf16': 0.018, 'small/int8k': 0.050, 'small/int8kv': 0.062, 'dyn16/int8kv': 0.019,
                   'reg6/int8k': 0.009}
C_BF16 = 6.84                  # 3 x 2.279 (generic decode kernel, head size 256); the cap for these classes is 8
C_INT8 = 0.19                  # 3 x 0.062 (small kernel, int8kv)
UNIT = 2.0 ** -20
# fp32 underflow, an absolute floor under the bound: a softmax weight, or its product with a cache scale, below 2^-126 is flushed to zero
# (the one-instruction exp2 returns no denormals), so each of at most 1088 keys can drop up to 2^-126 x 128 (the largest |byte - 128|; the
# bf16 values here are smaller).  It shows only where the reference itself is of that size: an 8-bit value cache whose heavy row holds byte
# 128 in a component (MI355X: out -1.987e-36 for ref -1.969e-36 at Tcap 256, t 128, int8kv, peaked).
UNDERFLOW = 1088 * 128 * 2.0 ** -126
OBSERVED = {}                  # filled by check(): largest observed c per (kernel class / cache format) in this process

FMTS = ('bf16', 'int8k', 'int8kv')
BYTE_POISON = 0x5A             # cache bytes of rows >= t
BYTE_GUARD = 0xC3              # guard bytes around a byte cache
INT_GUARD = -1010101           # guard words around the device-side step counter


def c_bound(fmt):
    return C_BF16 if fmt == 'bf16' else C_INT8


# ------------------------------------------------------------------------------------------------ the dispatcher's rule, restated
def decode_branch(rows, nh, E, Tcap, t_max, fmt='bf16', row_scale=1, force_long=False, long_split=None):
    """which kernel rq_launch_attn_decode picks (csrc/rqt_kernels.hip), from the same quantities: 'generic', 'small', 'reg<NJ>' /
    'reg<NJ>x2' (attn_decode_kernel<NJ, false, P>), 'dyn16' / 'dyn32' (<16 / 32, true, 1>), 'long4' / 'long1' (attn_long_kernel<NW>)"""
    if E != nh * 64:
        return 'generic'
    nj_cap = (Tcap + 7) // 8
    nj = min((t_max >> 3) + 1 if t_max >= 0 else nj_cap, nj_cap)
    big = rows * row_scale * nh
    if nj == 1:
        return 'small'
    if (force_long and fmt == 'bf16') or (Tcap > 256 and nj > 32):
        split = long_split if long_split is not None else big < 4096
        return 'long4' if split else 'long1'
    if Tcap > 256:
        return 'dyn16' if nj <= 16 else 'dyn32'
    if Tcap <= 64:
        two = nh % 2 == 0 and nj <= 4 and big >= 16384
        return 'reg%d%s' % (nj, 'x2' if two else '')
    return 'dyn16' if Tcap <= 128 else 'dyn32'


def prefill_branch(P, nh, E, fmt='bf16', force_tiled=False):
    """rq_launch_attn_prefill: 'generic', 'tiled' (attn_prefill_tiled_kernel), 'plain' (attn_prefill_kernel)"""
    if E != nh * 64:
        return 'generic'
    if P > 255 or (force_tiled and fmt == 'bf16'):
        return 'tiled'
    return 'plain'


def packed_branch(nh, E):
    """rq_launch_attn_packed: attn_packed_kernel<64, true> / <0, true> / <0, false>"""
    hd = E // nh
    return 'hd64' if hd == 64 else 'vec' if hd % 8 == 0 else 'scalar'


# ------------------------------------------------------------------------------------------------ buffers
class Buf:
    """`content` (a CPU tensor) inside a larger flat buffer on `dev` with poisoned guards on both sides: NaN around floating types
    (kernel_check.guarded), BYTE_GUARD around bytes.  .t is the view the kernel gets."""

    def __init__(self, content, dev):
        self.n = content.numel()
        self.pattern = None if content.dtype.is_floating_point else BYTE_GUARD if content.dtype == torch.uint8 else INT_GUARD
        if self.pattern is not None:
            buf = torch.full((self.n + 2 * GUARD,), self.pattern, dtype=content.dtype)
            buf[GUARD:GUARD + self.n] = content.reshape(-1)
            self.buf = buf.to(dev)
            self.t = self.buf[GUARD:GUARD + self.n].view(content.shape)
        else:
            self.buf, self.t = guarded(tuple(content.shape), content.dtype, dev)
            self.t.copy_(content)

    def check_guard(self, what):
        if self.pattern is not None:
            for part, name in ((self.buf[:GUARD], 'before'), (self.buf[GUARD + self.n:], 'after')):
                assert bool((part == self.pattern).all()), f'{what}: stores {name} the buffer'
        else:
            check_guard(self.buf, self.n, what)


def nan_like(shape, dtype=torch.bfloat16):
    return torch.full(tuple(shape), float('nan'), dtype=dtype)


def bits(t):
    """the raw bits of a tensor on the CPU (NaN payloads included)"""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ reference and bound
def attn_ref(q, K, V, mask=None):
    """fp64 (ref, A): q (..., nq, hd), K / V (..., nk, hd), mask (nq, nk) bool or None"""
    s = q @ K.transpose(-1, -2) * (1.0 / math.sqrt(q.shape[-1]))
    if mask is not None:
        s = s.masked_fill(~mask, float('-inf'))
    p = torch.softmax(s, dim=-1)
    return p @ V, p @ V.abs()


def check(out, ref, A, fmt, cls, what=''):
    """asserts the elementwise bound (NaN fails); records and returns the observed c = max (|err| - 1/2 ulp) / (2^-20 A)"""
    c = c_bound(fmt)
    out = out.to(ref.device).double().reshape(ref.shape)
    err = (out - ref).abs()
    half = 0.5 * bf16_ulp(ref) + UNDERFLOW
    unit = UNIT * A
    ratio = float(((err - half).clamp_min(0.0) / unit.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max())
    key = f'{cls}/{fmt}'
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), ratio)
    bad = ~(err <= half + c * unit)                       # NaN counts as bad
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f'{what} [{key}]: {int(bad.sum())} of {bad.numel()} outside the bound (observed c {ratio:.3f} > {c}); first at {i}: '
                             f'out {float(out[i])!r}, ref {float(ref[i])!r}, |err| {float(err[i]):.3e} > {float((half + c * unit)[i]):.3e}')
    return ratio


def report():
    return ', '.join('%s %.3f' % kv for kv in sorted(OBSERVED.items()))


def check_quant(k, b, s, what=''):
    """the 8-bit append of csrc/rqt_kernels.hip (quant_key_chunk): k (..., 64) the bf16 key or value, b (..., 64) its bytes, s (...) its
    scale.  Scale within 1 fp32 ulp of absmax / 127; |(byte - 128) scale - k| <= scale (0.5 + 2^-16) (the fp32 rounding of k * (127 / absmax)
    moves a component by at most 127 x 2^-23 of a step before rint); the absmax component maps to +-127; an all-zero key has scale 1.0 and
    bytes 128; a key with a NaN / inf component has a NaN scale and bytes 128."""
    k, b, s = k.detach().cpu().double(), b.detach().cpu().to(torch.int32) - 128, s.detach().cpu().double()
    fin = torch.isfinite(k).all(-1)
    am = k.abs().amax(-1)
    zero, norm = fin & (am == 0), fin & (am > 0)
    assert bool(torch.isnan(s[~fin]).all()) and bool((b[~fin] == 0).all()), f'{what}: a key with a NaN / inf component'
    assert bool((s[zero] == 1.0).all()) and bool((b[zero] == 0).all()), f'{what}: an all-zero key'
    kn, bn, sn, an = k[norm], b[norm], s[norm], am[norm]
    want = an / 127.0
    _, e = torch.frexp(want)
    ulp = torch.ldexp(torch.ones_like(want), e - 24)                     # fp32 ulp at want: want = m 2^e, m in [0.5, 1)
    assert bool(((sn - want).abs() <= ulp).all()), f'{what}: scale further than 1 fp32 ulp from absmax / 127'
    dq = bn.double() * sn[:, None]
    assert bool(((dq - kn).abs() <= sn[:, None] * (0.5 + 2.0 ** -16)).all()), f'{what}: a component further than half a step from its byte'
    top = kn.abs() == an[:, None]
    assert bool((bn[top] == (127 * torch.sign(kn[top])).to(torch.int32)).all()), f'{what}: the absmax component is not +-127'


# ------------------------------------------------------------------------------------------------ inputs
def _pick(lo, hi, g):
    """one integer per element in [lo, hi) (tensors, hi > lo)"""
    return lo + (torch.rand(lo.shape, generator=g) * (hi - lo)).floor().long().clamp(max=(hi - lo - 1).clamp_min(0))


class DecodeInput:
    pass


def make_decode(rows, nh, hd, Tcap, t, fmt, kind, seed):
    """inputs of one decode step at position t: q, k, v of this token and a cache whose rows < t hold random values (bf16, or bytes
    over 0 .. 255 with positive scales) and whose rows >= t hold poison.  'peaked': q = 8 x one key per (row, head) -- pair % 3 == 0: one
    of the first 8 keys, 1: one of the last 8 cached keys, 2: this token's own key (j = t).  'low' (bf16 cache): every key is one
    direction k0 + a little noise and q = -16 k0, so every score lies near -16 |k0|^2 / 8 ~ -128: the softmax is nearly flat, but only
    relative to a maximum whose exp underflows fp32 -- a partial (m, l) merged against a reference of 0 instead of the true maximum
    loses everything."""
    g = torch.Generator().manual_seed(seed)
    d = DecodeInput()
    d.rows, d.nh, d.hd, d.Tcap, d.t, d.fmt, d.E = rows, nh, hd, Tcap, t, fmt, nh * hd
    q, d.k, d.v = (torch.randn((rows, nh, hd), generator=g).bfloat16() for _ in range(3))

    def cache(as_bytes):
        if as_bytes:
            c = torch.randint(0, 256, (rows, nh, Tcap, 64), generator=g, dtype=torch.uint8)
            sc = ((0.5 + torch.rand((rows, nh, Tcap), generator=g)) / 73.0).float()           # components ~ unit variance
            c[:, :, t:] = BYTE_POISON
            sc[:, :, t:] = float('nan')
            return c, sc, (c[:, :, :t].double() - 128.0) * sc[:, :, :t, None].double()
        c = torch.randn((rows, nh, Tcap, hd), generator=g).bfloat16()
        c[:, :, t:] = float('nan')
        return c, None, c[:, :, :t].double()
    d.kc, d.ksc, kpast = cache(fmt != 'bf16')
    d.vc, d.vsc, vpast = cache(fmt == 'int8kv')
    if kind == 'low':                                                     # every key near one direction, q against it
        assert fmt == 'bf16'
        k0 = torch.randn((rows, nh, 1, hd), generator=g)
        d.kc[:, :, :t] = (k0 + 0.0625 * torch.randn((rows, nh, t, hd), generator=g)).bfloat16()
        d.k = (k0[:, :, 0] + 0.0625 * torch.randn((rows, nh, hd), generator=g)).bfloat16()
        q = (-16.0 * k0[:, :, 0]).bfloat16()
        kpast = d.kc[:, :, :t].double()
    d.K = torch.cat([kpast, d.k.double()[:, :, None]], dim=2)             # (rows, nh, t + 1, hd) fp64
    d.V = torch.cat([vpast, d.v.double()[:, :, None]], dim=2)
    if kind == 'peaked':
        pair = torch.arange(rows * nh).view(rows, nh)
        tt = torch.full((rows, nh), t)
        zero = torch.zeros_like(tt)
        first = _pick(zero, tt.clamp(max=8), g) if t > 0 else tt
        last = _pick((tt - 8).clamp_min(0), tt, g) if t > 0 else tt
        win = torch.where(pair % 3 == 0, first, torch.where(pair % 3 == 1, last, tt))
        kw = torch.gather(d.K, 2, win[:, :, None, None].expand(rows, nh, 1, hd))[:, :, 0]
        q = (8.0 * kw).float().bfloat16()
    else:
        assert kind in ('flat', 'low')
    d.q = q
    d.qkv = torch.cat([q.reshape(rows, -1), d.k.reshape(rows, -1), d.v.reshape(rows, -1)], dim=-1).contiguous()
    return d


def slice_decode(d, b):
    """row b of a decode input as an input of its own"""
    s = DecodeInput()
    s.__dict__.update(d.__dict__)
    s.rows = 1
    for name in ('q', 'k', 'v', 'kc', 'vc', 'ksc', 'vsc', 'K', 'V', 'qkv'):
        x = getattr(d, name)
        setattr(s, name, None if x is None else x[b:b + 1].contiguous())
    return s


class Run:
    pass


def run_decode(nat, dev, d, t_max, row_scale=1, step_base=None):
    r = Run()
    r.qkv, r.kc, r.vc = Buf(d.qkv, dev), Buf(d.kc, dev), Buf(d.vc, dev)
    r.ksc = Buf(d.ksc, dev) if d.ksc is not None else None
    r.vsc = Buf(d.vsc, dev) if d.vsc is not None else None
    r.y = Buf(nan_like((d.rows, d.E)), dev)
    r.step = Buf(torch.full((1,), -12345, dtype=torch.int32), dev) if step_base is not None else None
    r.t_max, r.row_scale, r.step_base = t_max, row_scale, step_base
    launch_decode(nat, d, r)
    return r


def launch_decode(nat, d, r):
    nat.dbg_set_row_scale(r.row_scale)
    try:
        nat.dbg_rqt_attn_decode(r.qkv.t, r.kc.t, r.vc.t, r.y.t, d.nh, d.Tcap, d.t, t_max=r.t_max, ksc=r.ksc.t if r.ksc else None,
                                vsc=r.vsc.t if r.vsc else None, step=r.step.t if r.step else None, step_base=r.step_base or 0)
    finally:
        nat.dbg_set_row_scale(1)


def _check_cache(buf, scale_buf, before, before_scale, new, t, what):
    """row t of every pair holds this token's `new` (rows, nh, hd); every other row is bit for bit what it was (rows > t: the poison)"""
    now = buf.t.cpu()
    if scale_buf is None:
        want = before.clone()
        want[:, :, t] = new
        assert same_bits(now, want), f'{what}: cache rows differ from (old rows, this token at row {t}, poison beyond)'
    else:
        now_s = scale_buf.t.cpu()
        keep = torch.arange(before.shape[2]) != t
        assert same_bits(now[:, :, keep], before[:, :, keep]), f'{what}: byte rows other than {t} changed'
        assert same_bits(now_s[:, :, keep], before_scale[:, :, keep]), f'{what}: scales other than row {t} changed'
        check_quant(new, now[:, :, t], now_s[:, :, t], what)
        scale_buf.check_guard(what + ' scales')
    buf.check_guard(what)


def verify_decode(d, r, cls, what):
    """output within the bound of the fp64 reference, every side effect bit for bit; returns the observed c"""
    dev = r.y.t.device
    ref, A = attn_ref(d.q.double().to(dev)[:, :, None], d.K.to(dev), d.V.to(dev))
    ratio = check(r.y.t.view(d.rows, d.nh, 1, d.hd), ref, A, d.fmt, cls, what)
    r.y.check_guard(what + ' y')
    r.qkv.check_guard(what + ' qkv')
    assert same_bits(r.qkv.t, d.qkv), f'{what}: qkv changed'
    _check_cache(r.kc, r.ksc, d.kc, d.ksc, d.k, d.t, what + ' K cache')
    _check_cache(r.vc, r.vsc, d.vc, d.vsc, d.v, d.t, what + ' V cache')
    if r.step is not None:
        assert int(r.step.t.cpu()[0]) == r.step_base, f'{what}: the step counter changed'
        r.step.check_guard(what + ' step')
    return ratio


def decode_case(nat, dev, rows, nh, Tcap, t, t_max, fmt='bf16', kind='flat', hd=64, row_scale=1, step_base=None, expect=None,
                force_long=False, long_split=None):
    """one decode launch, checked; `expect` names the kernel the case is meant for (asserted by the dispatcher's rule)"""
    got = decode_branch(rows, nh, nh * hd, Tcap, t_max, fmt, row_scale, force_long, long_split)
    assert got == expect, f'case meant for {expect} reaches {got}'
    what = f'decode {expect} rows {rows} nh {nh} hd {hd} Tcap {Tcap} t {t} t_max {t_max} {fmt} {kind} step {step_base}'
    d = make_decode(rows, nh, hd, Tcap, t, fmt, kind, seed=1 + 7 * t + 1009 * Tcap + 13 * rows + nh)
    r = run_decode(nat, dev, d, t_max, row_scale, step_base)
    verify_decode(d, r, expect, what)
    return d, r


class PrefillInput:
    pass


def make_prefill(n_img, P, nh, hd, kind, seed):
    """q, k, v (n_img, P, nh, hd) bf16.  'peaked': q_i = 8 k_j(i), j(i) among the first 64 keys (i % 3 == 0), the last 8 keys before i
    (1) or i itself (2)"""
    g = torch.Generator().manual_seed(seed)
    d = PrefillInput()
    d.n_img, d.P, d.nh, d.hd, d.E = n_img, P, nh, hd, nh * hd
    q, d.k, d.v = (torch.randn((n_img, P, nh, hd), generator=g).bfloat16() for _ in range(3))
    if kind == 'peaked':
        i = torch.arange(P)[None, :, None].expand(n_img, P, nh)
        first = _pick(torch.zeros_like(i), (i + 1).clamp(max=64), g)
        last = torch.where(i > 0, _pick((i - 8).clamp_min(0), i.clamp_min(1), g), i)
        win = torch.where(i % 3 == 0, first, torch.where(i % 3 == 1, last, i))
        q = (8.0 * torch.gather(d.k.float(), 1, win[..., None].expand(n_img, P, nh, hd))).bfloat16()
    else:
        assert kind == 'flat'
    d.q = q
    d.qkv = torch.cat([x.reshape(n_img * P, -1) for x in (q, d.k, d.v)], dim=-1).contiguous()
    return d


def prefill_ref(d, dev):
    q, k, v = (x.double().to(dev).permute(0, 2, 1, 3) for x in (d.q, d.k, d.v))          # (n_img, nh, P, hd)
    mask = torch.ones((d.P, d.P), dtype=torch.bool, device=dev).tril()
    ref, A = attn_ref(q, k, v, mask)
    return ref.permute(0, 2, 1, 3), A.permute(0, 2, 1, 3)                                   # (n_img, P, nh, hd)


def run_prefill(nat, dev, d, Tcap, fmt='bf16', cache=True):
    r = Run()
    r.qkv = Buf(d.qkv, dev)
    r.y = Buf(nan_like((d.n_img * d.P, d.E)), dev)
    r.kc = r.vc = r.ksc = r.vsc = None
    r.Tcap, r.fmt = Tcap, fmt
    if cache:
        shape = (d.n_img, d.nh, Tcap, d.hd)
        r.kc0 = nan_like(shape) if fmt == 'bf16' else torch.full(shape, BYTE_POISON, dtype=torch.uint8)
        r.vc0 = nan_like(shape) if fmt != 'int8kv' else torch.full(shape, BYTE_POISON, dtype=torch.uint8)
        r.kc, r.vc = Buf(r.kc0, dev), Buf(r.vc0, dev)
        r.ksc0 = r.vsc0 = nan_like(shape[:3], torch.float32)
        r.ksc = Buf(r.ksc0, dev) if fmt != 'bf16' else None
        r.vsc = Buf(r.vsc0, dev) if fmt == 'int8kv' else None
    nat.dbg_rqt_attn_prefill(r.qkv.t, r.y.t, d.n_img, d.P, d.nh, Tcap, kc=r.kc.t if r.kc else None, vc=r.vc.t if r.vc else None,
                             ksc=r.ksc.t if r.ksc else None, vsc=r.vsc.t if r.vsc else None)
    return r


def _check_prefill_cache(buf, scale_buf, before, before_scale, new, P, what):
    """rows 0 .. P-1 hold the tokens' `new` (n_img, P, nh, hd); rows P .. Tcap-1 are untouched"""
    now = buf.t.cpu()
    new = new.permute(0, 2, 1, 3)                                                          # (n_img, nh, P, hd)
    assert same_bits(now[:, :, P:], before[:, :, P:]), f'{what}: rows beyond the prefix changed'
    if scale_buf is None:
        assert same_bits(now[:, :, :P], new), f'{what}: rows 0 .. {P - 1} are not the tokens\' own'
    else:
        now_s = scale_buf.t.cpu()
        assert same_bits(now_s[:, :, P:], before_scale[:, :, P:]), f'{what}: scales beyond the prefix changed'
        check_quant(new, now[:, :, :P], now_s[:, :, :P], what)
        scale_buf.check_guard(what + ' scales')
    buf.check_guard(what)


def verify_prefill(d, r, cls, what, ref=None):
    dev = r.y.t.device
    ref, A = ref if ref is not None else prefill_ref(d, dev)
    ratio = check(r.y.t.view(d.n_img, d.P, d.nh, d.hd), ref, A, 'bf16', cls, what)       # (the prefix attention itself runs on bf16 k / v)
    r.y.check_guard(what + ' y')
    r.qkv.check_guard(what + ' qkv')
    assert same_bits(r.qkv.t, d.qkv), f'{what}: qkv changed'
    if r.kc is not None:
        _check_prefill_cache(r.kc, r.ksc, r.kc0, r.ksc0, d.k, d.P, what + ' K cache')
        _check_prefill_cache(r.vc, r.vsc, r.vc0, r.vsc0, d.v, d.P, what + ' V cache')
    return ratio


def prefill_case(nat, dev, n_img, P, nh, Tcap, fmt='bf16', cache=True, kind='flat', hd=64, expect=None, force_tiled=False, ref=None, d=None):
    got = prefill_branch(P, nh, nh * hd, fmt, force_tiled)
    assert got == expect, f'case meant for {expect} reaches {got}'
    what = f'prefill {expect} images {n_img} P {P} nh {nh} hd {hd} Tcap {Tcap} {fmt} cache {cache} {kind}'
    d = d if d is not None else make_prefill(n_img, P, nh, hd, kind, seed=3 + 31 * P + nh + 7 * hd)
    r = run_prefill(nat, dev, d, Tcap, fmt, cache)
    verify_prefill(d, r, expect, what, ref)
    return d, r


def packed_case(nat, dev, group, nh, hd, kind, expect):
    """groups of `group` rows, group * 33 rows in all"""
    E, rows = nh * hd, group * 33
    assert packed_branch(nh, E) == expect
    what = f'packed {expect} group {group} rows {rows} nh {nh} hd {hd} {kind}'
    d = make_prefill(33, group, nh, hd, kind, seed=5 + 11 * group + nh + 3 * hd)           # 33 sequences of `group` tokens
    qkv, y = Buf(d.qkv, dev), Buf(nan_like((rows, E)), dev)
    nat.dbg_rqt_attn_packed(qkv.t, y.t, group, nh)
    ref, A = prefill_ref(d, y.t.device)
    ratio = check(y.t.view(33, group, nh, hd), ref, A, 'bf16', 'packed-' + expect, what)
    y.check_guard(what + ' y')
    qkv.check_guard(what + ' qkv')
    assert same_bits(qkv.t, d.qkv), f'{what}: qkv changed'
    return ratio


# ------------------------------------------------------------------------------------------------ case lists
KINDS = ('flat', 'peaked')
SMALL_ROWS = (3, 7)                                                  # x nh 5: 15 pairs (one partial wavefront), 35 (two workgroups, clamped tail)
REG_TMAX = (8, 15, 16, 23, 24, 31, 32, 39, 40, 47, 48, 55, 56, 63)
# (Tcap, t, t_max) of the register kernel at Tcap <= 64
REG_CASES = [(64, tm, tm) for tm in REG_TMAX] + [(64, 8, 63), (64, 62, 63), (60, 59, 59)]
# (Tcap, t, t_max, formats): Tcap <= 128 -> <16, true>, <= 256 -> <32, true>; beyond 256 by t_max, bf16 only
DYN_CASES = ([(100, t, 99, FMTS) for t in (8, 63, 64, 99)] + [(128, 127, 127, FMTS), (200, 199, 199, FMTS)]
             + [(256, t, 255, FMTS) for t in (128, 255)] + [(320, 100, 100, ('bf16',)), (320, 255, 255, ('bf16',))])
LONG_T = {320: (63, 64, 191, 192, 255, 256, 257, 319), 1088: (511, 512, 1087)}
LONG_T_EMU = {320: LONG_T[320], 1088: (512, 1087)}                   # the emulator file trims Tcap 1088 to these
GENERIC_HD = (20, 32, 80, 128, 256)
GENERIC_T = (0, 1, 63, 64, 65, 255)
PREFILL_PLAIN = (1, 2, 63, 64, 65, 128, 129, 255)
PREFILL_TILED = (256, 257, 320)
PREFILL_INT8 = (2, 65, 255)
PREFILL_FORCED = (65, 129, 255)
PREFILL_GENERIC = [(hd, P) for hd in (20, 80) for P in (1, 64, 65, 256)]
PACKED = [(hd, nh) for hd in (64, 32, 20) for nh in (1, 5)]


def small_cases(nat, dev, rows, fmt):
    """attn_small_kernel: t = 0 .. 7 under t_max = 7, t by value and through a device counter"""
    for t in range(8):
        for kind in KINDS:
            decode_case(nat, dev, rows, 5, 11, t, 7, fmt, kind, expect='small')
        if t >= 2:
            decode_case(nat, dev, rows, 5, 11, t, 7, fmt, 'flat', step_base=t - 2, expect='small')


def reg_cases(nat, dev, fmt, two):
    """attn_decode_kernel<NJ, false, P>: nh 5 at row scale 1 (one head per wavefront, idle wavefronts in the last workgroup), nh 6 at row
    scale 4096 (two heads per wavefront while t_max <= 31)"""
    for Tcap, t, t_max in REG_CASES:
        nj = (t_max >> 3) + 1
        if two and t_max > 31:
            continue
        for kind in KINDS:
            decode_case(nat, dev, 3, 6 if two else 5, Tcap, t, t_max, fmt, kind, row_scale=4096 if two else 1,
                        step_base=t - 3 if kind == 'peaked' else None, expect='reg%d%s' % (nj, 'x2' if two else ''))


def dyn_cases(nat, dev, fmt):
    for Tcap, t, t_max, fmts in DYN_CASES:
        if fmt not in fmts:
            continue
        nj = min((t_max >> 3) + 1, (Tcap + 7) // 8)
        expect = ('dyn16' if nj <= 16 else 'dyn32') if Tcap > 256 else 'dyn16' if Tcap <= 128 else 'dyn32'
        for kind in KINDS:
            decode_case(nat, dev, 3, 5, Tcap, t, t_max, fmt, kind, step_base=5 if kind == 'peaked' else None, expect=expect)


def long_cases(nat, dev, Tcap, nw, ts):
    """attn_long_kernel<NW>: NW = 4 at row scale 1 (t = 63 leaves three wavefronts without a chunk), NW = 1 at row scale 4096"""
    for t in ts:
        for kind in KINDS:
            decode_case(nat, dev, 2, 3, Tcap, t, Tcap - 1, 'bf16', kind, row_scale=1 if nw == 4 else 4096,
                        step_base=t - 40 if kind == 'peaked' else None, expect='long%d' % nw)


def long_low_cases(nat, dev, nw):
    """the chunked kernel on scores that all lie near -128 (kind 'low'): t = 63 and 100 leave three and two of the four wavefronts of the
    NW = 4 form without a chunk, t = 319 none"""
    for t in (63, 100, 319):
        decode_case(nat, dev, 2, 3, 320, t, 319, 'bf16', 'low', row_scale=1 if nw == 4 else 4096, expect='long%d' % nw)


def generic_cases(nat, dev, hd):
    for t in GENERIC_T:
        for kind in KINDS:
            decode_case(nat, dev, 2, 3, 256, t, 255, 'bf16', kind, hd=hd, step_base=0 if kind == 'peaked' else None, expect='generic')


def prefill_cases(nat, dev, P, expect):
    """with a cache of exactly P rows, of P + 9 rows, and cache-free"""
    d = make_prefill(2, P, 3, 64, 'flat', seed=3 + 31 * P)
    ref = prefill_ref(d, dev)
    for Tcap, cache in ((P, True), (P + 9, True), (P, False)):
        prefill_case(nat, dev, 2, P, 3, Tcap, cache=cache, expect=expect, d=d, ref=ref)
    prefill_case(nat, dev, 2, P, 3, P + 9, kind='peaked', expect=expect)


def prefill_forced_tiled(nat, dev, P, setenv):
    """RQAMD_PREFILL_TILED=1 below 256 tokens: outputs and cache rows bit-identical to attn_prefill_kernel, as the source claims"""
    d = make_prefill(2, P, 3, 64, 'peaked', seed=17 + P)
    ref = prefill_ref(d, dev)
    setenv('RQAMD_PREFILL_TILED', '0')
    _, a = prefill_case(nat, dev, 2, P, 3, P + 9, expect='plain', d=d, ref=ref)
    setenv('RQAMD_PREFILL_TILED', '1')
    _, b = prefill_case(nat, dev, 2, P, 3, P + 9, expect='tiled', force_tiled=True, d=d, ref=ref)
    assert same_bits(a.y.t, b.y.t), f'P {P}: the tiled kernel\'s output differs from the plain kernel\'s'
    assert same_bits(a.kc.t, b.kc.t) and same_bits(a.vc.t, b.vc.t), f'P {P}: cache rows differ'
    _, c = prefill_case(nat, dev, 2, P, 3, P, cache=False, expect='tiled', force_tiled=True, d=d, ref=ref)
    assert same_bits(a.y.t, c.y.t), f'P {P}: the cache-free tiled form differs'


def special_keys(rows, nh, g):
    """k / v (rows, nh, 64) bf16 whose first pairs are: all zero, one NaN, one +inf, one -inf, a single non-zero component, a component of 2^127
    (quant_key_chunk counts an absmax above 3.0e38 as not finite); the rest N(0, 1) x a spread of magnitudes"""
    x = torch.randn((rows * nh, 64), generator=g) * torch.logspace(-30, 30, rows * nh, base=2.0)[:, None]
    x[0] = 0.0
    x[1, 5] = float('nan')
    x[2, 63] = float('inf')
    x[3, 0] = float('-inf')
    x[4] = 0.0
    x[4, 17] = -3.0
    x[5, 9] = 2.0 ** 127
    return x.view(rows, nh, 64).bfloat16()


def append_special(nat, dev, fmt):
    """the 8-bit append on keys / values with zero, NaN, inf and extreme components, through the small kernel (t = 3), the register kernel
    (t = 9) and the prefill kernel; the same k / v gives identical bytes and scales through all three (outputs are not judged: a
    non-finite key makes its pair's output NaN by definition)"""
    g = torch.Generator().manual_seed(99)
    rows, nh = 3, 5
    k, v = special_keys(rows, nh, g), special_keys(rows, nh, g).flip(0)
    got = {}
    for t, t_max, expect in ((3, 7, 'small'), (9, 15, 'reg2')):
        assert decode_branch(rows, nh, nh * 64, 16, t_max, fmt) == expect
        d = make_decode(rows, nh, 64, 16, t, fmt, 'flat', seed=t)
        d.k, d.v = k, v
        d.qkv = torch.cat([d.q.reshape(rows, -1), k.reshape(rows, -1), v.reshape(rows, -1)], dim=-1).contiguous()
        r = run_decode(nat, dev, d, t_max)
        what = f'append {expect} {fmt}'
        _check_cache(r.kc, r.ksc, d.kc, d.ksc, k, t, what + ' K cache')
        _check_cache(r.vc, r.vsc, d.vc, d.vsc, v, t, what + ' V cache')
        r.y.check_guard(what)
        got[expect] = tuple(x.t.cpu()[:, :, t] if x is not None else None for x in (r.kc, r.ksc, r.vc, r.vsc))
    # the same keys as token 1 of a two-token prefix
    d = make_prefill(rows, 2, nh, 64, 'flat', seed=4)
    d.k[:, 1], d.v[:, 1] = k, v
    d.qkv = torch.cat([x.reshape(rows * 2, -1) for x in (d.q, d.k, d.v)], dim=-1).contiguous()
    r = run_prefill(nat, dev, d, 5, fmt)
    _check_prefill_cache(r.kc, r.ksc, r.kc0, r.ksc0, d.k, 2, f'append prefill {fmt} K cache')
    _check_prefill_cache(r.vc, r.vsc, r.vc0, r.vsc0, d.v, 2, f'append prefill {fmt} V cache')
    got['plain'] = tuple(x.t.cpu()[:, :, 1] if x is not None else None for x in (r.kc, r.ksc, r.vc, r.vsc))
    for name in ('reg2', 'plain'):
        for a, b in zip(got['small'], got[name]):
            assert (a is None) == (b is None) and (a is None or same_bits(a, b)), f'{fmt}: small and {name} appends differ'


def chain_vs_prefill(nat, dev):
    """decode steps t = 0 .. 70 over one cache (Tcap 128) against one prefill of the same 71 tokens: caches bit-identical, outputs each
    within the bound of the same reference"""
    n, P, nh, Tcap = 2, 71, 3, 128
    d = make_prefill(n, P, nh, 64, 'flat', seed=71)
    ref, A = prefill_ref(d, dev)
    _, rp = prefill_case(nat, dev, n, P, nh, Tcap, expect='plain', d=d, ref=(ref, A))
    kc, vc = Buf(nan_like((n, nh, Tcap, 64)), dev), Buf(nan_like((n, nh, Tcap, 64)), dev)
    E = nh * 64
    for t in range(P):
        expect = decode_branch(n, nh, E, Tcap, t)
        assert expect == ('small' if t < 8 else 'dyn16')
        qkv = Buf(torch.cat([x[:, t].reshape(n, -1) for x in (d.q, d.k, d.v)], dim=-1).contiguous(), dev)
        y = Buf(nan_like((n, E)), dev)
        nat.dbg_rqt_attn_decode(qkv.t, kc.t, vc.t, y.t, nh, Tcap, t, t_max=t)
        check(y.t.view(n, nh, 64), ref[:, t], A[:, t], 'bf16', 'chain-' + expect, f'chained decode step {t}')
        y.check_guard(f'chained decode step {t}')
    assert same_bits(kc.t, rp.kc.t) and same_bits(vc.t, rp.vc.t), 'the chained decode steps and the prefill leave different caches'
    kc.check_guard('chain K cache')
    vc.check_guard('chain V cache')


# (name, keyword arguments of decode_case at rows = 3): one per kernel class, for the row-independence and relaunch checks
CLASS_CASES = [
    ('small', dict(nh=5, Tcap=11, t=5, t_max=7)),
    ('reg3', dict(nh=5, Tcap=64, t=20, t_max=23)),
    ('reg2x2', dict(nh=6, Tcap=64, t=13, t_max=15, row_scale=4096 * 3)),
    ('dyn16', dict(nh=5, Tcap=100, t=70, t_max=99)),
    ('dyn32', dict(nh=5, Tcap=200, t=150, t_max=199)),
    ('long4', dict(nh=3, Tcap=320, t=200, t_max=319)),
    ('long1', dict(nh=3, Tcap=320, t=200, t_max=319, row_scale=4096)),
    ('generic', dict(nh=3, Tcap=256, t=70, t_max=255, hd=80)),
]


def rows_and_relaunch(nat, dev, name, kw):
    """row b of a 3-row launch is bit-identical to the 1-row launch on that row in the same kernel class, and a second launch on the same
    buffers reproduces output and caches bit for bit"""
    kw = dict(kw)
    hd, scale = kw.pop('hd', 64), kw.pop('row_scale', 1)
    d, r = decode_case(nat, dev, 3, kind='peaked', hd=hd, row_scale=scale, expect=name, **kw)
    y1, k1, v1 = r.y.t.clone(), r.kc.t.clone(), r.vc.t.clone()
    r.y.t.fill_(float('nan'))
    launch_decode(nat, d, r)
    assert same_bits(r.y.t, y1) and same_bits(r.kc.t, k1) and same_bits(r.vc.t, v1), f'{name}: a second launch differs'
    assert decode_branch(1, kw['nh'], kw['nh'] * hd, kw['Tcap'], kw['t_max'], 'bf16', scale) == name
    for b in range(3):
        s = slice_decode(d, b)
        rs = run_decode(nat, dev, s, kw['t_max'], scale)
        assert same_bits(rs.y.t, y1[b:b + 1]), f'{name}: row {b} alone differs from row {b} of the 3-row launch'
        assert same_bits(rs.kc.t, k1[b:b + 1]) and same_bits(rs.vc.t, v1[b:b + 1])


def forced_long_vs_register(nat, dev, setenv):
    """RQAMD_ATTN_LONG=1 at Tcap 64, t 40: attn_long_kernel on a context the register kernel serves -- within the bound, the same cache, and
    no further from the register kernel's output than both bounds allow"""
    kw = dict(rows=3, nh=5, Tcap=64, t=40, t_max=63, kind='peaked')
    setenv('RQAMD_ATTN_LONG', '0')
    d, a = decode_case(nat, dev, expect='reg8', **kw)
    setenv('RQAMD_ATTN_LONG', '1')
    _, b = decode_case(nat, dev, expect='long4', force_long=True, **kw)
    assert same_bits(a.kc.t, b.kc.t) and same_bits(a.vc.t, b.vc.t)
    ref, A = attn_ref(d.q.double().to(dev)[:, :, None], d.K.to(dev), d.V.to(dev))
    diff = (a.y.t.double() - b.y.t.double()).abs().view(ref.shape)
    assert bool((diff <= bf16_ulp(ref) + 2 * C_BF16 * UNIT * A).all())
    setenv('RQAMD_ATTN_LONG_SPLIT', '0')
    decode_case(nat, dev, expect='long1', force_long=True, long_split=False, **kw)
    return float(diff.max())


def refusals(nat, dev, pytest):
    """the launchers' own refusals pass through the entries with their messages; nothing is launched"""
    def dec(rows=2, nh=3, hd=64, Tcap=320, t=10, t_max=100, fmt='bf16'):
        d = make_decode(rows, nh, hd, Tcap, t, fmt, 'flat', seed=1)
        return run_decode(nat, dev, d, t_max)
    for fmt in ('int8k', 'int8kv'):
        for t_max in (100, 255, 319):
            with pytest.raises(NotImplementedError, match='end at 256 keys'):
                dec(fmt=fmt, t_max=t_max)
    with pytest.raises(NotImplementedError, match='head_dim 257 > 256'):
        dec(hd=257, Tcap=16, t_max=15)
    with pytest.raises(NotImplementedError, match='context 257 > 256'):
        dec(hd=80, Tcap=257, t_max=256)
    with pytest.raises(NotImplementedError, match='written for head_dim 64'):
        d = make_decode(2, 3, 64, 16, 3, 'int8k', 'flat', seed=1)
        d.qkv, d.E = torch.zeros((2, 3 * 240), dtype=torch.bfloat16), 240                  # head size 80 with key scales
        run_decode(nat, dev, d, 15)

    def pre(P=4, Tcap=8, fmt='bf16', cache=True, hd=64, stray=False):
        d = make_prefill(2, P, 3, hd, 'flat', seed=2)
        if not stray:
            return run_prefill(nat, dev, d, Tcap, fmt, cache)
        qkv, y, vc = Buf(d.qkv, dev), Buf(nan_like((2 * P, d.E)), dev), Buf(nan_like((2, 3, Tcap, hd)), dev)
        return nat.dbg_rqt_attn_prefill(qkv.t, y.t, 2, P, 3, Tcap, vc=vc.t)
    for fmt in ('int8k', 'int8kv'):
        with pytest.raises(NotImplementedError, match='end at 255 prefix tokens'):
            pre(P=256, Tcap=256, fmt=fmt)
    with pytest.raises(NotImplementedError, match=r'9 tokens \(cache 8\)'):
        pre(P=9)
    with pytest.raises(NotImplementedError, match=r'9 tokens \(cache 8\)'):
        pre(P=9, hd=20)
    with pytest.raises(ValueError, match='cache-free form with a cache pointer'):
        pre(stray=True)
    with pytest.raises(NotImplementedError, match='context 257 > 256'):
        pre(P=4, Tcap=257, hd=20)

    def pack(rows, group, nh=2, hd=64):
        qkv, y = Buf(torch.zeros((rows, 3 * nh * hd), dtype=torch.bfloat16), dev), Buf(nan_like((rows, nh * hd)), dev)
        nat.dbg_rqt_attn_packed(qkv.t, y.t, group, nh)
    with pytest.raises(ValueError, match='18 rows in groups of 9'):
        pack(18, 9)
    with pytest.raises(ValueError, match='17 rows in groups of 4'):
        pack(17, 4)
    with pytest.raises(NotImplementedError, match='head_dim 257 > 256'):
        pack(8, 4, nh=1, hd=257)
