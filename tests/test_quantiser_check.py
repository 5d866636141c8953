"""CPU self-test of tests/quantiser_check.py, the certificate checker of the quantiser tests (tests/test_gpu_quantiser.py,
tests/test_emu_quantiser.py): it accepts the oracle's codes, torch's fp32 distances and the sequential fp32 chain at C_CHAIN, and
rejects each way the kernel could go subtly wrong -- the second-nearest code on one row, the later index of a duplicate pair, one
code's norm taken from its neighbour, one dropped dimension pair, a code >= K, quants summed in reverse depth order, one store into
a guard, distances that are right relative to the matrix maximum but wrong on its smallest entry.  It also re-measures C_CHAIN and
KAPPA on the reference side and holds the case lists to the launch forms and ring-step classes they claim.  This is the evidence
that the GPU tests can fail."""
import numpy as np
import pytest
import torch

import kernel_check as kc
import oracle
import quantiser_check as qc

T = torch.from_numpy


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def _fp32_distances(x, cb, cn=None, drop=None):
    """the expanded form in torch fp32; cn: the code norms to use, drop: dims left out of r.c"""
    xn = (x * x).sum(1)
    cn = (cb * cb).sum(1) if cn is None else cn
    keep = torch.ones(x.shape[1], dtype=torch.bool)
    if drop is not None:
        keep[list(drop)] = False
    return (xn[:, None] + cn[None]) - 2.0 * (x[:, keep] @ cb[:, keep].T)


@pytest.fixture(scope='module')
def case():
    """2000 vectors against 64 codes at dim 64 (small gaps exist: a mutated distance flips some codes), and the oracle's codes over
    four depths of one codebook"""
    rng = np.random.default_rng(21)
    cb = rng.standard_normal((64, 64), dtype=np.float32)
    x = rng.standard_normal((2000, 64), dtype=np.float32)
    _, codes = oracle.rq_quantize(x, [cb] * 4)
    return T(x), T(cb), T(codes)


def test_accepts_the_oracles_codes_and_quants(case):
    x, cb, codes = case
    assert qc.check_codes(x, [cb] * 4, codes) < 1.0
    qc.check_ties([cb] * 4, codes)
    assert qc.ambiguous_share(x, [cb] * 4, codes) <= 0.01 and qc.ambiguous_share(x, [cb] * 4) <= 0.01
    assert torch.equal(qc.reference_codes(x, [cb] * 4), codes)
    oq, _ = oracle.rq_quantize(x.numpy(), [cb.numpy()] * 4)
    qc.check_quants(T(np.stack(oq)), [cb] * 4, codes)
    qc.check_embed(T(oracle.rq_embed_code(codes.numpy(), [cb.numpy()] * 4)), 0, [cb] * 4, codes)
    qc.check_embed(T(oracle.rq_embed_code_with_depth(codes.numpy(), [cb.numpy()] * 4)), 1, [cb] * 4, codes)
    qc.check_embed(T(np.stack(oq, 1)), 2, [cb] * 4, codes)
    for case_ in qc.SINGLE_CASES[:4] + qc.SPLIT_CASES[2:3]:                 # K = 1 and K < 4 included
        xs, cbs = qc.make_case(case_)
        _, oc = oracle.rq_quantize(xs, cbs)
        qc.check_codes(T(xs), [T(c) for c in cbs], T(oc), case_.name)


def test_accepts_fp32_distances_and_the_chain_at_c_chain(case):
    x, cb, _ = case
    assert qc.check_distances(_fp32_distances(x, cb), x, cb, 1.0) < qc.C_CHAIN[64]
    qc.check_distances(T(oracle.compute_distances(x.numpy(), cb.numpy())), x, cb, qc.C_CHAIN[64])
    qc.check_distances(T(qc.chain_distances(x.numpy(), cb.numpy())), x, cb, qc.C_CHAIN[64])
    qc.check_norms((cb * cb).sum(1), cb)
    _rejects(lambda: qc.check_norms((cb * cb).sum(1) * (1 + 2e-5), cb))


def test_c_chain_and_kappa_are_four_times_the_reference_side_measurements():
    """the recorded values are what the helpers measure on the cases' own inputs (rounded up by < 1 %), and the constants 4 x them"""
    for recorded, measured in ((qc.CHAIN_MEASURED, qc.measure_chain()), (qc.KAPPA_MEASURED, qc.measure_kappa())):
        assert sorted(recorded) == sorted(measured) == [64, 128, 192, 256]
        for dim, v in measured.items():
            assert 0.99 * recorded[dim] <= v <= recorded[dim], (dim, v, recorded[dim])
    assert qc.C_CHAIN == {d: 4.0 * v for d, v in qc.CHAIN_MEASURED.items()} and max(qc.C_CHAIN.values()) < 1.0
    assert qc.KAPPA == {d: 4.0 * v for d, v in qc.KAPPA_MEASURED.items()}


def test_rejects_the_second_nearest_code_on_one_row(case):
    x, cb, codes = case
    d64, S = qc.dist_ref(x, cb)
    E = qc.err_bound(S, 64)
    top2 = d64.topk(2, dim=1, largest=False)
    gap = top2.values[:, 1] - top2.values[:, 0]
    ok = gap > E.gather(1, top2.indices).sum(1)                             # gap beyond E[k] + E[second]
    i = int(torch.where(ok, gap, torch.full_like(gap, float('inf'))).argmin())      # the row where it is hardest to see
    bad = codes.clone()
    bad[i, 0] = top2.indices[i, 1]
    _rejects(lambda: qc.check_codes(x, [cb] * 4, bad))
    _rejects(lambda: qc.check_codes(x, [cb], bad[:, :1]))


def test_rejects_the_later_index_of_a_duplicate_pair():
    tcase = qc.EMU_TIE_CASES[0]
    x, cbs = qc.make_case(tcase)
    x, cbs = T(x), [T(c) for c in cbs]
    codes = qc.reference_codes(x, cbs)
    assert np.array_equal(codes[:, 0].numpy(), qc.tie_targets(tcase))       # torch.argmin: the first minimum
    qc.check_codes(x, cbs, codes)
    qc.check_ties(cbs, codes)
    for lo, hi in tcase.ties:
        bad = codes.clone()
        rows = (bad[:, 0] == lo).nonzero()[:, 0]
        bad[rows[0], 0] = hi
        qc.check_codes(x, cbs, bad)                                         # equal distances: the certificate cannot see it
        _rejects(lambda: qc.check_ties(cbs, bad))
    xs, same = qc.make_case(qc.EMU_TIE_CASES[2])
    zero = torch.zeros((xs.shape[0], 2), dtype=torch.int64)
    qc.check_ties([T(c) for c in same], zero)
    zero[3, 1] = 129
    _rejects(lambda: qc.check_ties([T(c) for c in same], zero))


def test_rejects_a_norm_taken_from_the_neighbouring_code(case):
    x, cb, codes = case
    cn = (cb * cb).sum(1)
    j = int((cn[:-1] - cn[1:]).argmax())                                    # code j gets the smaller norm of code j + 1
    wrong = cn.clone()
    wrong[j] = cn[j + 1]
    d = _fp32_distances(x, cb, cn=wrong)
    _rejects(lambda: qc.check_distances(d, x, cb, 1.0))
    got = d.argmin(1)
    assert int((got != codes[:, 0]).sum()) > 0
    _rejects(lambda: qc.check_codes(x, [cb], got[:, None]))


def test_rejects_a_dropped_dimension_pair(case):
    x, cb, codes = case
    d = _fp32_distances(x, cb, drop=(38, 39))
    _rejects(lambda: qc.check_distances(d, x, cb, 1.0))
    got = d.argmin(1)
    assert int((got != codes[:, 0]).sum()) > 0
    _rejects(lambda: qc.check_codes(x, [cb], got[:, None]))


def test_rejects_a_code_out_of_range(case):
    x, cb, codes = case
    for v in (64, -1, 0x7fffffff):
        bad = codes.clone()
        bad[1999, 3] = v
        _rejects(lambda: qc.check_codes(x, [cb] * 4, bad))
        _rejects(lambda: qc.check_quants(qc.quants_ref([cb] * 4, codes), [cb] * 4, bad))
        _rejects(lambda: qc.check_ties([cb] * 4, bad))


def test_rejects_quants_summed_in_reverse_depth_order(case):
    x, cb, codes = case
    e = [cb[codes[:, d]] for d in range(4)]
    rev = torch.stack([e[0], e[1] + e[0], e[2] + (e[1] + e[0]), e[3] + (e[2] + (e[1] + e[0]))])      # the same sums, still depth order
    qc.check_quants(rev, [cb] * 4, codes)
    rev[3] = ((e[3] + e[2]) + e[1]) + e[0]
    assert not torch.equal(rev[3], qc.quants_ref([cb] * 4, codes)[3])
    _rejects(lambda: qc.check_quants(rev, [cb] * 4, codes))
    _rejects(lambda: qc.check_embed(rev[3], 0, [cb] * 4, codes))
    _rejects(lambda: qc.check_embed(rev.permute(1, 0, 2).contiguous(), 2, [cb] * 4, codes))
    _rejects(lambda: qc.check_embed(torch.cumsum(torch.stack(e, 1), 1), 1, [cb] * 4, codes))


def test_rejects_a_store_into_a_guard(case):
    x, cb, codes = case
    for where in (0, qc.GUARD - 1, qc.GUARD + codes.numel(), 2 * qc.GUARD + codes.numel() - 1):
        buf, out = qc.guarded_codes(codes.shape, 'cpu')
        out.copy_(codes)
        qc.check_code_guard(buf, out.numel())
        buf[where] = 0
        _rejects(lambda: qc.check_code_guard(buf, out.numel()))
    buf, out = kc.guarded((4, 2000, 64), torch.float32, 'cpu')
    out.copy_(qc.quants_ref([cb] * 4, codes))
    kc.check_guard(buf, out.numel())
    buf[kc.GUARD + out.numel()] = 0.0
    _rejects(lambda: kc.check_guard(buf, out.numel()))


def test_rejects_distances_wrong_on_the_smallest_entry_only():
    """residual-like inputs: an error of 2e-5 of the matrix maximum (what the older tests allowed) on the smallest entry.  At dim 256
    that is just inside the derived ceiling c = 1 there (r ~ c: S ~ 4 |c|^2, E ~ 0.016); the measured C_CHAIN is what sees it."""
    x, cbs = qc.make_case(qc.SINGLE_CASES[-1])
    x, cb = T(x), T(cbs[0])
    d = _fp32_distances(x, cb)
    qc.check_distances(d, x, cb, qc.C_CHAIN[256])
    i = int(d.argmin())
    bad = d.clone()
    bad.view(-1)[i] += 2e-5 * float(d.max())
    assert float((bad - d).abs().max()) <= 2e-5 * float(d.max())
    _rejects(lambda: qc.check_distances(bad, x, cb, qc.C_CHAIN[256]))
    bad.view(-1)[i] += 2e-5 * float(d.max())
    _rejects(lambda: qc.check_distances(bad, x, cb, 1.0))


def test_soft_code_check():
    """accepts the fp32 softmax of fp32 distances, rejects a row normalised over the wrong sum and one probability off by 1e-4 of itself"""
    scase = qc.SOFT_CASES[0]
    x, cbs = qc.make_case(scase)
    x, cbs = T(x), [T(c) for c in cbs]
    temp, kappa = qc.soft_temp(scase.dim), qc.KAPPA[scase.dim]
    codes = qc.reference_codes(x, cbs)
    soft = torch.stack([qc.soft_fp32(_fp32_distances(r, cbs[d]).double(), temp) for d, r in qc.forced_residuals(x, cbs, codes)], 1)
    assert qc.check_soft(soft, x, cbs, codes, temp, kappa) <= 1.0
    bad = soft.clone()
    bad[7, 1] *= 1.0 + 1e-4
    _rejects(lambda: qc.check_soft(bad, x, cbs, codes, temp, kappa))
    bad = soft.clone()
    k = int(soft[9, 0].argmin())
    bad[9, 0, k] *= 1.0 + 1e-2                                                   # invisible in the row sum and in any absolute tolerance
    _rejects(lambda: qc.check_soft(bad, x, cbs, codes, temp, kappa))


def test_case_lists_reach_the_launch_forms_they_claim():
    every = qc.SINGLE_CASES + qc.SPLIT_CASES + qc.TIE_CASES + qc.DIST_CASES + qc.SOFT_CASES + qc.EMU_CASES + qc.EMU_TIE_CASES
    assert len({c.name for c in every}) == len(every)
    for c in qc.SINGLE_CASES + qc.SPLIT_CASES + qc.TIE_CASES + qc.EMU_CASES + qc.EMU_TIE_CASES:
        plan = qc.split_plan(c.n_vec, c.ks)
        assert (plan is not None) == c.split, c.name
        assert qc.split_plan(c.n_vec, c.ks, 96) is None, c.name              # dbg_set_row_scale(96): the single launch
    for cases in (qc.SINGLE_CASES, qc.SPLIT_CASES, qc.EMU_CASES):
        assert {c.dim for c in cases} == {64, 128, 192, 256}
    steps = {qc.nstep(K, c.dim) for c in qc.SINGLE_CASES for K in c.ks}
    assert {1, 2, 3, 4} <= steps and max(steps) > 4
    assert {1, 2, 3} <= {qc.nstep(K, c.dim) for c in qc.EMU_CASES for K in c.ks}
    assert {c.n_vec for c in qc.SINGLE_CASES} >= {1, 63, 64, 65, 130}
    assert {c.n_vec for c in qc.SPLIT_CASES} >= {1, 70, 6016}
    assert {K for c in qc.SPLIT_CASES for K in c.ks} >= {1024, 1025, 1153, 2304, 8190}
    by = {c.name: c for c in every}
    assert qc.split_plan(6016, (1025,)) == [(2, 5)]                              # tiles 8 alone in the last split, one code in it
    assert qc.split_plan(5, (8190,)) == [(1, 64)] and 8190 % 128 != 0            # the 64-split cap, ragged last tile
    assert qc.split_plan(70, (1100, 1100, 1300)) == [(1, 9), (1, 9), (2, 6)]     # n_split recomputed per depth
    t = by['ties_split']
    (tps, n_split), = set(qc.split_plan(t.n_vec, t.ks))
    assert tps == 2 and (t.ks[0] - 1) // 128 // tps == n_split - 1 and (t.ks[0] - 1) % 128 == 0
    gaps = {hi - lo for lo, hi in t.ties}
    assert gaps >= {1, 32, 128, tps * 128, t.ks[0] - 1}
    lo, hi = [p for p in t.ties if p[1] - p[0] == 128][0]
    assert lo // 128 // tps == hi // 128 // tps and lo // 128 != hi // 128      # next tile, same split
    lo, hi = [p for p in t.ties if p[1] - p[0] == tps * 128][0]
    assert lo // 128 // tps + 1 == hi // 128 // tps                             # next split
    for c in qc.TIE_CASES + qc.EMU_TIE_CASES:
        if c.kind == 'ties':
            _, cbs = qc.make_case(c)
            first = qc.first_equal_row(T(cbs[0]))
            assert all(first[hi] == lo for lo, hi in c.ties) and (first != np.arange(c.ks[0])).sum() == len(c.ties)


def test_certificate_power_of_every_case():
    """check 2 on the reference side, for the cases small enough for the CPU (the GPU tests assert it for every case along the kernel's
    own codes)"""
    for c in qc.SINGLE_CASES + qc.EMU_CASES + [s for s in qc.SPLIT_CASES if s.n_vec <= 70]:
        x, cbs = qc.make_case(c)
        assert qc.ambiguous_share(T(x), [T(b) for b in cbs]) <= 0.01, c.name
