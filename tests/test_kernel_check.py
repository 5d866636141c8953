"""CPU self-test of tests/kernel_check.py, the strict checker of the GPU kernel tests (tests/test_gpu_gemm_conv.py): it accepts the
correctly rounded bf16 / fp32 results and torch's own fp32 matmul, and rejects each way a kernel goes subtly wrong -- truncation
instead of round-to-nearest-even, one dropped K-tile, a wrong last ragged row or column, bias missing or doubled on one column, one
store into the guard, a slab holding the wrong K range, the wrong padding of a stride-2 conv, a bias error in the sub-pixel form of
the upsample conv -- at the loosest c of any family.  This is the evidence that the GPU tests can fail."""
import pytest
import torch
import torch.nn.functional as F

import kernel_check as kc

C_LOOSE = max(kc.C.values())
C_TIGHT = min(kc.C.values())


@pytest.fixture(scope='module')
def case():
    g = torch.Generator().manual_seed(11)
    M, N, K = 67, 83, 1024                              # ragged against every tile
    a = torch.randn((M, K), generator=g).to(torch.bfloat16)
    w = (torch.randn((N, K), generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn((N,), generator=g)
    ref, S = kc.gemm_ref(a, w, bias)
    return a, w, bias, ref, S


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_accepts_rounded_and_torch_results(case):
    a, w, bias, ref, S = case
    n = kc.steps(a.shape[1])
    kc.check_f32(ref.float(), ref, S, n, C_TIGHT)
    kc.check_f32(a.float() @ w.float().T + bias, ref, S, n, C_TIGHT)
    kc.check_bf16(ref.float().to(torch.bfloat16), ref, S, n, C_TIGHT)
    kc.check_bf16(ref.to(torch.bfloat16), ref, S, n, C_TIGHT)
    kc.check_bf16(kc.gelu64(ref).float().to(torch.bfloat16), ref, S, n, C_TIGHT, gelu=True)
    buf, out = kc.guarded(ref.shape, torch.float32, 'cpu')
    out.copy_(ref.float())
    kc.check_guard(buf, out.numel())


def test_rejects_truncation(case):
    a, w, bias, ref, S = case
    n = kc.steps(a.shape[1])
    _rejects(lambda: kc.check_bf16(kc.round_bf16_trunc(ref), ref, S, n, C_LOOSE))
    _rejects(lambda: kc.check_bf16(kc.round_bf16_trunc(kc.gelu64(ref)), ref, S, n, C_LOOSE, gelu=True))


def test_rejects_a_dropped_k_tile(case):
    a, w, bias, ref, S = case
    n = kc.steps(a.shape[1])
    drop, _ = kc.gemm_ref(a, w, None, 5 * 64, 6 * 64)
    bad = (ref - drop).float()
    _rejects(lambda: kc.check_f32(bad, ref, S, n, C_LOOSE))
    _rejects(lambda: kc.check_bf16(bad.to(torch.bfloat16), ref, S, n, C_LOOSE))


def test_rejects_a_wrong_last_row_or_column(case):
    a, w, bias, ref, S = case
    n = kc.steps(a.shape[1])
    for mutate in (lambda t: t[-1].copy_(t[-2]), lambda t: t[:, -1].copy_(t[:, -2]), lambda t: t[-1].zero_(), lambda t: t[:, -1].zero_()):
        bad = ref.float().clone()
        mutate(bad)
        _rejects(lambda: kc.check_f32(bad, ref, S, n, C_LOOSE))
        _rejects(lambda: kc.check_bf16(bad.to(torch.bfloat16), ref, S, n, C_LOOSE))


def test_rejects_bias_missing_or_doubled_on_one_column(case):
    a, w, bias, ref, S = case
    n = kc.steps(a.shape[1])
    j = int(bias.abs().argmin())                       # the column where it is hardest to see
    assert abs(float(bias[j])) > 1e-3
    for f in (-1.0, 1.0):
        bad = ref.float().clone()
        bad[:, j] += f * bias[j]
        _rejects(lambda: kc.check_f32(bad, ref, S, n, C_LOOSE))
    j = int(bias.abs().argmax())
    bad = ref.float().clone()
    bad[:, j] -= bias[j]
    _rejects(lambda: kc.check_bf16(bad.to(torch.bfloat16), ref, S, n, C_LOOSE))


def test_rejects_a_store_into_the_guard(case):
    a, w, bias, ref, S = case
    for where in (0, kc.GUARD - 1, kc.GUARD + ref.numel(), kc.GUARD * 2 + ref.numel() - 1):
        buf, out = kc.guarded(ref.shape, torch.float32, 'cpu')
        out.copy_(ref.float())
        buf[where] = 0.0
        _rejects(lambda: kc.check_guard(buf, out.numel()))
    slabs = torch.full((8, 4, 4), float('nan'))
    slabs[5, 3, 3] = 1.0
    _rejects(lambda: kc.check_nan(slabs[4:]))


def test_rejects_a_slab_with_the_wrong_k_range(case):
    a, w, bias, ref, S = case
    K = a.shape[1]
    kk = K // 4
    slabs = [kc.gemm_ref(a, w, None, z * kk, (z + 1) * kk) for z in range(4)]
    for z, (r, s) in enumerate(slabs):
        kc.check_f32(r.float(), r, s, kc.steps(kk, 4, 0), C_TIGHT)
    r1, s1 = slabs[1]
    _rejects(lambda: kc.check_f32(slabs[2][0].float(), r1, s1, kc.steps(kk, 4, 0), C_LOOSE))
    shifted, _ = kc.gemm_ref(a, w, None, kk + 64, 2 * kk + 64)             # off by one K-tile
    _rejects(lambda: kc.check_f32(shifted.float(), r1, s1, kc.steps(kk, 4, 0), C_LOOSE))


def test_conv_reference_and_padding():
    """the im2col reference equals torch's conv (stride 1, the folded upsample, stride 2 with the reference's (0, 1, 0, 1) pad), and a
    stride-2 conv padded on all sides is rejected"""
    g = torch.Generator().manual_seed(12)
    x = torch.randn((2, 8, 6, 64), generator=g).to(torch.bfloat16)
    w = (torch.randn((32, 3, 3, 64), generator=g) / 24).to(torch.bfloat16)
    bias = torch.randn((32,), generator=g)
    xt, wt = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    n = kc.steps(9 * 64)
    for stride, ups in ((1, 0), (1, 1), (2, 0)):
        xi = xt.repeat_interleave(2, 2).repeat_interleave(2, 3) if ups else xt
        xi = F.pad(xi, (0, 1, 0, 1)) if stride == 2 else xi
        want = F.conv2d(xi, wt, bias.double(), stride=stride, padding=0 if stride == 2 else 1).permute(0, 2, 3, 1).reshape(-1, 32)
        ref, S, _ = kc.conv_ref(x, w, bias, stride=stride, ups=ups)
        assert torch.allclose(ref, want, rtol=0, atol=1e-12)
        kc.check_bf16(want.to(torch.bfloat16), ref, S, n, C_TIGHT)
    ref, S, _ = kc.conv_ref(x, w, bias, stride=2)
    sym = F.conv2d(xt, wt, bias.double(), stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, 32)
    _rejects(lambda: kc.check_bf16(sym.to(torch.bfloat16), ref, S, n, C_LOOSE))


def test_bf16_ulp_from_the_exponent():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, -3.0, 2.0 ** -126, 0.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133], dtype=torch.float64)
    assert torch.equal(kc.bf16_ulp(x), want)
    # every bf16 value's neighbour is one ulp away
    v = torch.tensor([1.0, 3.0, 0.01, 100.0], dtype=torch.bfloat16)
    nxt = (v.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal(nxt.double() - v.double(), kc.bf16_ulp(v.double()))


def test_subpixel_reference_and_its_bias():
    """the sub-pixel reference (four 2 x 2 convs over the source image) with the exact fp64 tap sums equals the folded-upsample conv;
    with the bf16-rounded taps a kernel would use, a result with the bias missing or doubled on the median-|bias| column is rejected"""
    g = torch.Generator().manual_seed(13)
    xs = torch.randn((2, 8, 6, 128), generator=g).to(torch.bfloat16)
    w = (torch.randn((64, 3, 3, 128), generator=g) / (9 * 128) ** 0.5).to(torch.bfloat16)
    bias = torch.randn((64,), generator=g)
    want, _, _ = kc.conv_ref(xs, w, bias, ups=1)
    ref, _ = kc.subpixel_conv_ref(xs, kc.subpixel_taps64(w), bias)
    assert torch.allclose(ref, want, rtol=0, atol=1e-12)
    wsub = kc.subpixel_taps64(w).float().to(torch.bfloat16)
    ref, S = kc.subpixel_conv_ref(xs, wsub, bias)
    n = kc.steps(4 * 128)
    kc.check_bf16(ref.to(torch.bfloat16), ref, S, n, C_TIGHT)
    j = int(bias.abs().argsort()[32])
    for f in (-1.0, 1.0):
        bad = ref.clone()
        bad[:, j] += f * bias[j].double()
        _rejects(lambda: kc.check_bf16(bad.to(torch.bfloat16), ref, S, n, C_LOOSE))
