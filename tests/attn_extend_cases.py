"""Shared by tests/test_emu_attn_extend.py (host emulator) and tests/test_gpu_attn_extend.py (MI355X): the stand-alone checks of the
cache-extending causal attention (csrc/rqt_attn_extend.hip) through rqamd_dbg_rqt_attn_extend.

The kernel's claim is that the R outputs and the R appended cache rows are bit for bit those of the prefill kernels over all T0 + R
tokens -- the kernels tests/rqt_attn_cases.py holds against fp64.  So the certificate has two parts:

  1. bit-identity   rqamd_dbg_rqt_attn_prefill over T0 + R tokens per image, against -- on fresh buffers -- rqamd_dbg_rqt_attn_prefill over
                    the first T0 tokens followed by rqamd_dbg_rqt_attn_extend over the remaining R: the y rows of the R tokens and cache
                    rows 0 .. T0+R-1 equal in bits.  (T0 + R <= 255 meets the plain prefill kernel, beyond that the tiled one.)
  2. fp64           one direct check per Tcap against attn_ref with the bound and C_BF16 of rqt_attn_cases.py, class 'extend/bf16', on the
                    'flat', 'peaked' and 'low' inputs.

Observed c on MI355X (class extend/bf16): 0.114 on the 'flat' inputs and 0.000 on the 'peaked' ones -- where the 'tiled' (0.062) and
'plain' (0.064) classes of rqt_attn_cases.py sit on other seeds; on equal inputs part 1 makes the bits equal -- and 6.293 on the 'low' inputs
(Tcap 64; 5.083 / 4.482 / 2.093 at Tcap 256 / 384 / 1088), a kind the prefill classes are not run on: every score lies near -128 behind a
64-term sequential fp32 dot product, the situation of the 'generic' (2.279) and 'long' (1.981) decode classes.  The bound is C_BF16 = 6.84.

Buffers as there: qkv, caches and y inside larger buffers with NaN guards, cache rows >= T0 NaN before the launch (a read of one becomes a
NaN in y), y NaN.  Nothing here reaches a trap: the kernel has none, and the refusals are host-side."""
import torch

import rqt_attn_cases as R

NH, E = 2, 128
# (Tcap, T0, R, n_img)
CASES = [(64, 1, 1, 3), (64, 5, 2, 3), (64, 17, 47, 3), (256, 63, 64, 3), (256, 64, 65, 3), (256, 65, 3, 3), (384, 250, 70, 3),
         (1088, 1000, 88, 1)]
CASES_F16 = [c for c in CASES if c[0] in (64, 384)]
# one direct fp64 check per Tcap
FP64_CASES = [(64, 17, 47, 3), (256, 64, 65, 3), (384, 250, 70, 3), (1088, 1000, 88, 1)]
KINDS = ('flat', 'peaked', 'low')
OBSERVED_MI355X = {'extend/bf16': 6.293}      # the 'low' inputs at Tcap 64; flat 0.114, peaked 0.000


def case_id(c):
    return 'Tcap%d-T0_%d-R%d' % c[:3]


def make_inputs(n_img, P, kind, seed):
    """q, k, v (n_img, P, NH, 64) bf16 of P tokens per image: 'flat' / 'peaked' as rqt_attn_cases.make_prefill; 'low' as make_decode's:
    every key of an (image, head) near one direction k0 and q = -16 k0, so every score lies near -128"""
    if kind != 'low':
        return R.make_prefill(n_img, P, NH, 64, kind, seed)
    g = torch.Generator().manual_seed(seed)
    d = R.PrefillInput()
    d.n_img, d.P, d.nh, d.hd, d.E = n_img, P, NH, 64, E
    k0 = torch.randn((n_img, 1, NH, 64), generator=g)
    d.k = (k0 + 0.0625 * torch.randn((n_img, P, NH, 64), generator=g)).bfloat16()
    d.v = torch.randn((n_img, P, NH, 64), generator=g).bfloat16()
    d.q = (-16.0 * k0).expand(n_img, P, NH, 64).bfloat16().contiguous()
    d.qkv = torch.cat([x.reshape(n_img * P, -1) for x in (d.q, d.k, d.v)], dim=-1).contiguous()
    return d


def _rows(d, lo, hi, dt):
    """the qkv rows of tokens lo .. hi-1 of every image, (n_img * (hi - lo), 3E)"""
    return d.qkv.view(d.n_img, d.P, 3 * E)[:, lo:hi].reshape(-1, 3 * E).contiguous().to(dt)


class ExtendRun:
    pass


def run_split(nat, dev, d, Tcap, T0, Rn, half=False):
    """fresh NaN caches; prefill over the first T0 tokens, then the extend launch over the remaining Rn.  Returns the buffers and the
    caches' bits between the two launches"""
    dt = torch.float16 if half else torch.bfloat16
    r = ExtendRun()
    shape = (d.n_img, NH, Tcap, 64)
    r.kc, r.vc = R.Buf(R.nan_like(shape, dt), dev), R.Buf(R.nan_like(shape, dt), dev)
    r.qkv0, r.y0 = R.Buf(_rows(d, 0, T0, dt), dev), R.Buf(R.nan_like((d.n_img * T0, E), dt), dev)
    nat.dbg_rqt_attn_prefill(r.qkv0.t, r.y0.t, d.n_img, T0, NH, Tcap, kc=r.kc.t, vc=r.vc.t, half=half)
    r.k_mid, r.v_mid = r.kc.t.cpu().clone(), r.vc.t.cpu().clone()
    assert bool(torch.isnan(r.k_mid[:, :, T0:].float()).all()) and not bool(torch.isnan(r.k_mid[:, :, :T0].float()).any())
    r.qkv_in = _rows(d, T0, T0 + Rn, dt)
    r.qkv, r.y = R.Buf(r.qkv_in, dev), R.Buf(R.nan_like((d.n_img * Rn, E), dt), dev)
    nat.dbg_rqt_attn_extend(r.qkv.t, r.kc.t, r.vc.t, r.y.t, d.n_img, Rn, T0, NH, Tcap, half=half)
    return r


def check_side_effects(r, T0, Rn, what):
    """all guards intact, cache rows < T0 unchanged in bits, rows >= T0 + R still poison, qkv unchanged, no NaN in y"""
    for b, name in ((r.kc, 'K cache'), (r.vc, 'V cache'), (r.y, 'y'), (r.qkv, 'qkv')):
        b.check_guard(f'{what} {name}')
    assert R.same_bits(r.qkv.t, r.qkv_in), f'{what}: qkv changed'
    for now, mid, name in ((r.kc.t.cpu(), r.k_mid, 'K'), (r.vc.t.cpu(), r.v_mid, 'V')):
        assert R.same_bits(now[:, :, :T0], mid[:, :, :T0]), f'{what}: {name} cache rows < T0 changed'
        assert R.same_bits(now[:, :, T0 + Rn:], mid[:, :, T0 + Rn:]), f'{what}: {name} cache rows >= T0 + R changed'
        assert bool(torch.isnan(now[:, :, T0 + Rn:].float()).all())
        assert not bool(torch.isnan(now[:, :, T0:T0 + Rn].float()).any()), f'{what}: {name} rows of the run not written'
    assert not bool(torch.isnan(r.y.t.float()).any()), f'{what}: NaN in y (a cache row >= T0 was read, or a row was not written)'


def bit_identity(nat, dev, case, kind='flat', half=False):
    """part 1 of the certificate, with the side-effect checks of the extend launch"""
    Tcap, T0, Rn, n_img = case
    P = T0 + Rn
    dt = torch.float16 if half else torch.bfloat16
    what = f'extend {case_id(case)} images {n_img} {kind} {"fp16" if half else "bf16"}'
    d = make_inputs(n_img, P, kind, seed=11 + 31 * P + Tcap)
    full = ExtendRun()
    shape = (n_img, NH, Tcap, 64)
    full.kc, full.vc = R.Buf(R.nan_like(shape, dt), dev), R.Buf(R.nan_like(shape, dt), dev)
    full.qkv, full.y = R.Buf(d.qkv.to(dt), dev), R.Buf(R.nan_like((n_img * P, E), dt), dev)
    nat.dbg_rqt_attn_prefill(full.qkv.t, full.y.t, n_img, P, NH, Tcap, kc=full.kc.t, vc=full.vc.t, half=half)
    r = run_split(nat, dev, d, Tcap, T0, Rn, half)
    check_side_effects(r, T0, Rn, what)
    y_full = full.y.t.view(n_img, P, E)[:, T0:]
    assert R.same_bits(r.y.t.view(n_img, Rn, E), y_full), f'{what}: y differs from the prefill over all {P} tokens'
    assert R.same_bits(r.kc.t[:, :, :P], full.kc.t[:, :, :P]), f'{what}: K cache rows 0 .. {P - 1} differ'
    assert R.same_bits(r.vc.t[:, :, :P], full.vc.t[:, :, :P]), f'{what}: V cache rows 0 .. {P - 1} differ'
    return d, r


def fp64_check(nat, dev, case, kind):
    """part 2: the R outputs against attn_ref over all T0 + R keys, bound and constant of rqt_attn_cases; returns the observed c"""
    Tcap, T0, Rn, n_img = case
    P = T0 + Rn
    what = f'extend {case_id(case)} images {n_img} {kind} vs fp64'
    d = make_inputs(n_img, P, kind, seed=5 + 17 * P + Tcap)
    r = run_split(nat, dev, d, Tcap, T0, Rn)
    check_side_effects(r, T0, Rn, what)
    ydev = r.y.t.device
    q, k, v = (x.double().to(ydev).permute(0, 2, 1, 3) for x in (d.q, d.k, d.v))             # (n_img, NH, P, 64)
    mask = torch.ones((P, P), dtype=torch.bool, device=ydev).tril()[T0:]
    ref, A = R.attn_ref(q[:, :, T0:], k, v, mask)
    return R.check(r.y.t.view(n_img, Rn, NH, 64), ref.permute(0, 2, 1, 3), A.permute(0, 2, 1, 3), 'bf16', 'extend', what)


def refusals(nat, dev, pytest):
    """every refusal of include/rqamd.h, before any launch: the buffers are small and a launch with these sizes would be seen in the guards"""
    def bufs(n_img=2, Rn=3, nh=NH, hd=64, Tcap=16):
        Ee = nh * hd
        return (R.Buf(torch.zeros((n_img * Rn, 3 * Ee), dtype=torch.bfloat16), dev), R.Buf(R.nan_like((n_img, nh, Tcap, hd)), dev),
                R.Buf(R.nan_like((n_img, nh, Tcap, hd)), dev), R.Buf(R.nan_like((n_img * Rn, Ee)), dev))

    def call(n_img=2, Rn=3, T0=4, nh=NH, Tcap=16, hd=64, drop=None, b=None):
        b = b or bufs(n_img if n_img > 0 else 2, Rn if Rn > 0 else 3, nh if nh > 0 else NH, hd, Tcap if 0 < Tcap <= 16 else 16)
        t = [x.t for x in b]
        if drop is not None:
            t[drop] = None
        try:
            if drop == 0:                                         # (the binding reads E off qkv: pass the numbers straight)
                with nat.on_device_of(t[3]):
                    nat.check(nat.lib().rqamd_dbg_rqt_attn_extend(None, nat.ptr(t[1]), nat.ptr(t[2]), n_img, Rn, T0, nh, nh * hd, Tcap, nat.ptr(t[3]),
                                                                  nat.stream_of(t[3])))
            else:
                nat.dbg_rqt_attn_extend(t[0], t[1], t[2], t[3], n_img, Rn, T0, nh, Tcap)
        except (ValueError, NotImplementedError):
            for x in b:
                x.check_guard('refused extend launch')
            assert bool(torch.isnan(b[3].t.float()).all()) and bool(torch.isnan(b[1].t.float()).all()), 'a refused call launched'
            raise
        for x in b:
            x.check_guard('accepted extend launch')
        return b
    for drop in range(4):
        with pytest.raises(ValueError, match='null pointer'):
            call(drop=drop)
    for kw in (dict(n_img=0), dict(nh=0), dict(Rn=0), dict(T0=0), dict(Rn=-1), dict(T0=-5)):
        with pytest.raises(ValueError, match='each >= 1'):
            call(**kw)
    with pytest.raises(ValueError, match=r'14 cached \+ 3 new tokens \(cache 16\)'):
        call(T0=14)
    with pytest.raises(ValueError, match=r'new tokens \(cache 2\)'):
        call(Tcap=2, T0=1)
    with pytest.raises(NotImplementedError, match='head size 64 only'):
        call(hd=32)
    with pytest.raises(NotImplementedError, match='head size 64 only'):
        call(hd=80)
    with pytest.raises(NotImplementedError, match='RQAMD_RQT_MAX_CONTEXT'):
        call(Tcap=1089, T0=4)
    b = call(T0=13)                                               # (ends exactly at Tcap: accepted; rows 13 .. 15 hold the zero k / v of the qkv rows)
    assert bool((b[1].t[:, :, 13:] == 0).all()) and bool(torch.isnan(b[1].t[:, :, :13].float()).all())
