"""Min-p and locally typical sampling on the MI355X (`pytest -m gpu`): the TRUNC builds of the sampler kernels through
rqamd_sample_logits_trunc -- every case of tests/trunc_sampling_cases.py in the register and the general form, each stage certified
against fp64 on the kernel's own earlier kept set, per-row tables, the guided form, refusals -- and rqamd_rqt_sample_trunc through
RQTransformer.sample / sample_guided on the tiny fixture model: identity and graph accounting, membership of every drawn code,
graph == eager == cached=False, per-image values, log-probabilities, masks and guidance.  Run with -s for the observed maxima (copied
to profiles/trunc_sampling_certificate.txt)."""
import numpy as np
import pytest
import torch

import guided_sampling_cases as G
import masked_sampling_cases as M
import sampler_check as sc
import trunc_sampling_cases as tc
from oracle import configs as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 3
KW = dict(temperature=0.9, top_k=tc.ENGINE_TOP_K, top_p=tc.ENGINE_TOP_P)
TR = dict(min_p=tc.ENGINE_MIN_P, typical_p=tc.ENGINE_TYP)


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    yield _native
    for key in sorted(tc.OBSERVED):
        print(f'\ntrunc sampling: {key:28s} largest observed {tc.OBSERVED[key]:.4g}', end='')
    print(f'\ntrunc sampling: C_RACE_T {tc.C_RACE_T} u; probability, min-p and typical bounds as derived (c = 1)')


# ---------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize('case', tc.CASES, ids=lambda c: c.name)
def test_trunc_case(nat, case):
    out = tc.run_case(nat, case, DEV)
    print(f'{case.name}: largest deficit {out["worst"]:.3g} u, runner-up inside the tolerance in {out["near"]} of {out["rows"]} rows, '
          f'{out["band"]} entries inside the min-p band, forms that keep other sets in {out["diff"]} rows')
    if case.name.startswith('cap_'):
        # k = SMP_CAP distinct keys stay in the register form, k = SMP_CAP + 1 are handed to the general form
        assert (out['flags'] == int(case.k > sc.SMP_CAP)).all()
    if case.name == 'hard_k10_V16384':
        assert out['flags'][9] == 1 and out['flags'][10] == 1      # the two-valued row past SMP_CAP and the NaN threshold: handed back


@pytest.mark.parametrize('V', [16384, 500, 499, 7])
def test_trunc_rows(nat, V):
    """per-row tables that mix off and on rows: off rows bit-identical to rqamd_sample_logits_rows, on rows to the scalar call"""
    tc.run_rows_case(nat, V, DEV, None, what=f'rows V{V}')
    seeds = [3, 2 ** 40 + 5, 3, 0, 7, 2 ** 62, 1, 2 ** 63 + 11, 2 ** 32, 2 ** 32 - 1, 15, 17]
    tc.run_rows_case(nat, V, DEV, seeds, 99, 2 ** 32 + 1, f'row seeds V{V}')


@pytest.mark.parametrize('name', ['V500_k62_all', 'V16384_k2048_all', 'V499_koff_minp_typ', 'V16388_koff_typ'])
def test_trunc_guided(nat, name):
    case = next(c for c in tc.CASES if c.name == name)
    tc.run_guided_case(nat, case._replace(rows=min(case.rows, 8)), DEV)


def test_trunc_refusals(nat):
    tc.check_refusals(nat, DEV)


# ---------------------------------------------------------------------------------------------- engine level
@pytest.fixture(scope='module')
def tiny(nat):
    """RQT_TINY (4x4x4, V 500) with seeded weights, 3 images; sample() takes (SEED, OFFSET) in place of the generator's state"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    ar._draw_rng = lambda device, n: (tc.SEED, tc.OFFSET)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond)


def _zeros(b=B):
    return torch.zeros((b, 4, 4, 4), dtype=torch.long, device=DEV)


def test_engine_identity_and_graph_accounting(nat):
    """off values return the plain call's codes; alternating armed and unarmed calls captures nothing after the first of each"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)                # a model of its own: no graph of an earlier test
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    ar._draw_rng = lambda device, n: (tc.SEED, tc.OFFSET)
    eng = ar._eng(False)
    plain = ar.sample(_zeros(), aux, cond=cond, **KW)
    n0 = eng.graph_captures()
    assert n0 > 0
    for off in (dict(min_p=None, typical_p=None), dict(min_p=0), dict(min_p=0.0, typical_p=1.0), dict(typical_p=[1.0, -1.0, 1.0, 2.0]),
                dict(min_p=[0.0] * 4)):
        assert torch.equal(ar.sample(_zeros(), aux, cond=cond, **KW, **off), plain), off
        with ar.truncation(**off):
            assert torch.equal(ar.sample(_zeros(), aux, cond=cond, **KW), plain), off
    assert eng.graph_captures() == n0, 'an off value captured graphs of its own'
    a = ar.sample(_zeros(), aux, cond=cond, **KW, **TR)
    n1 = eng.graph_captures()
    assert n1 > n0 and not torch.equal(a, plain)
    for _ in range(2):
        assert torch.equal(ar.sample(_zeros(), aux, cond=cond, **KW), plain)
        assert torch.equal(ar.sample(_zeros(), aux, cond=cond, **KW, **TR), a)
    assert eng.graph_captures() == n1, 'alternating armed and unarmed calls recaptured'
    with ar.truncation(**TR):
        assert torch.equal(ar.sample(_zeros(), aux, cond=cond, **KW), a)
    # the per-image form: a new set of values replays the same graphs
    mp = torch.tensor([[0.05, 0.0, 0.3, 0.02]] * B, device=DEV)
    b1 = ar.sample(_zeros(), aux, cond=cond, **KW, min_p=mp, typical_p=0.9)
    n2 = eng.graph_captures()
    b2 = ar.sample(_zeros(), aux, cond=cond, **KW, min_p=mp * 0.5, typical_p=torch.tensor([0.5, 0.9, 0.2], device=DEV))
    assert eng.graph_captures() == n2 and b1.shape == b2.shape
    assert torch.equal(ar.sample(_zeros(), aux, cond=cond, **KW, **TR), a) and eng.graph_captures() == n2
    saved, ar.sampler = ar.sampler, 'torch'
    try:
        with pytest.raises(NotImplementedError):
            ar.sample(_zeros(), aux, cond=cond, **KW, min_p=0.1)
    finally:
        ar.sampler = saved
    for bad in (dict(min_p=1.5), dict(min_p=float('nan')), dict(typical_p=float('inf')), dict(min_p=[0.1, 0.2])):
        with pytest.raises(ValueError):
            ar.sample(_zeros(), aux, cond=cond, **KW, **bad)
    assert torch.equal(ar.sample(_zeros(), aux, cond=cond, **KW), plain)       # nothing stays armed after a refusal


def test_engine_membership(nat, tiny):
    """every drawn code lies in a kept set the certificates accept and wins the fp64 race on it; at most 1 % of the draws need a
    boundary tolerance; min_p = 0.3 excludes a code that the same seed draws without it"""
    ar, aux, cond, _ = tiny
    out = ar.sample(_zeros(), aux, cond=cond, **KW, **TR)
    logits = tc.masked_logits(ar, ar.teacher_forced_logits(out, aux, cond=cond)).cpu().numpy()
    n, tol = tc.engine_membership(nat, out.cpu().numpy(), logits, 0.9, tc.ENGINE_TOP_K, tc.ENGINE_TOP_P, tc.ENGINE_MIN_P, tc.ENGINE_TYP,
                                  tc.SEED, tc.OFFSET, DEV, what='sample')
    print(f'sample: {n} codes certified, {tol} needed a boundary tolerance')
    assert n == B * 64 and tol <= 0.01 * n
    plain = ar.sample(_zeros(), aux, cond=cond, **KW)
    mp = [0.3] * 4
    cut = ar.sample(_zeros(), aux, cond=cond, **KW, min_p=0.3)
    lp = tc.masked_logits(ar, ar.teacher_forced_logits(plain, aux, cond=cond)).cpu().numpy()
    where = tc.first_excluded(nat, plain.cpu().numpy(), cut.cpu().numpy(), lp, 0.9, tc.ENGINE_TOP_K, tc.ENGINE_TOP_P, mp, tc.SEED, tc.OFFSET, DEV)
    assert where is not None, 'min_p = 0.3 changed no draw of 192'
    print(f'min_p 0.3: the plain call\'s code at (position, depth, image) {where} lies outside the min-p set')


@pytest.mark.parametrize('amp', [False, True], ids=['bf16', 'fp16'])
def test_engine_paths(nat, tiny, amp):
    """graph == eager == cached=False; prefix_mode = 'one_pass' leaves the given prefix alone and draws from the same filters"""
    ar, aux, cond, _ = tiny
    a = ar.sample(_zeros(), aux, cond=cond, amp=amp, **KW, **TR)
    ar.use_graph = False
    try:
        b = ar.sample(_zeros(), aux, cond=cond, amp=amp, **KW, **TR)
    finally:
        ar.use_graph = True
    assert torch.equal(a, b), 'graph and eager calls differ'
    if not amp:
        c = ar.sample(_zeros(), aux, cond=cond, cached=False, **KW, **TR)
        assert torch.equal(a, c), 'cached=False differs from the cached call'
    given = G.random_codes((B, 4, 4, 4), 500, 3, DEV)
    s1 = ar.sample(given, aux, cond=cond, start_loc=(2, 1), amp=amp, **KW, **TR)
    saved, ar.prefix_mode = ar.prefix_mode, 'one_pass'
    try:
        s2 = ar.sample(given, aux, cond=cond, start_loc=(2, 1), amp=amp, **KW, **TR)
        ar.use_graph = False
        s3 = ar.sample(given, aux, cond=cond, start_loc=(2, 1), amp=amp, **KW, **TR)
    finally:
        ar.prefix_mode, ar.use_graph = saved, True
    assert torch.equal(s1.view(B, 16, 4)[:, :9], given.view(B, 16, 4)[:, :9]) and torch.equal(s2.view(B, 16, 4)[:, :9], given.view(B, 16, 4)[:, :9])
    # the one-pass prefix changes GEMM tiles, so the logits differ in their last bits and a draw may differ from the
    # stepped mode's where it was close (and everything after it); filters, Philox counters and captured graphs are the same
    assert torch.equal(s2, s3), 'one_pass: graph and eager calls differ'
    print(f'one_pass against stepped ({"fp16" if amp else "bf16"}): {100 * float((s1 == s2).float().mean()):.1f} % of the codes equal')


def test_engine_per_image(nat, tiny):
    """image b of a (B, D) call under seeds() == row 0 of the scalar call seeded with b's seed, with b's values as per-depth lists"""
    ar, aux, cond, _ = tiny
    mp = torch.tensor([[0.05, 0.0, 0.3, 0.02], [0.0, 0.0, 0.0, 0.0], [0.5, 0.1, 0.0, 1.0]], device=DEV)
    ty = torch.tensor([[0.9, 0.8, 1.0, 0.5], [0.2, 1.0, 0.9, 0.0], [1.0, 1.0, 1.0, 1.0]], device=DEV)
    seeds = [11, 2 ** 40 + 5, 11]
    saved = ar.__dict__.pop('_draw_rng')
    try:
        with ar.seeds(seeds):
            got = ar.sample(_zeros(), aux, cond=cond, **KW, min_p=mp, typical_p=ty)
            again = ar.sample(_zeros(), aux, cond=cond, **KW, min_p=mp, typical_p=ty, cached=False)
        assert torch.equal(got, again), 'cached=False differs from the cached per-image call'
        assert not torch.equal(got[0], got[2])
        for b in range(B):
            order = torch.tensor([b] + [i for i in range(B) if i != b], device=DEV)
            M.seed_all(seeds[b])
            want = ar.sample(_zeros(), aux, cond=cond[order].contiguous(), **KW, min_p=mp[b].tolist(), typical_p=ty[b].tolist())
            assert torch.equal(got[b], want[0]), f'image {b} is not row 0 of the scalar call with its values'
        # (B,) tensors broadcast over the depths
        with ar.seeds(seeds):
            v = ar.sample(_zeros(), aux, cond=cond, **KW, min_p=torch.tensor([0.1, 0.0, 0.3], device=DEV))
        M.seed_all(seeds[0])
        assert torch.equal(v[0], ar.sample(_zeros(), aux, cond=cond, **KW, min_p=0.1)[0])
    finally:
        ar._draw_rng = saved


def test_engine_log_probs(nat, tiny):
    """lp.draw == log of probs_out of rqamd_sample_logits_trunc on the same logits at the drawn code; +0.0 where one token survives;
    the same codes armed and unarmed"""
    ar, aux, cond, _ = tiny
    plain = ar.sample(_zeros(), aux, cond=cond, **KW, **TR)
    with ar.return_log_probs():
        codes, lp = ar.sample(_zeros(), aux, cond=cond, **KW, **TR)
    assert torch.equal(codes, plain)
    logits = tc.masked_logits(ar, ar.teacher_forced_logits(codes, aux, cond=cond))
    draw, cd = lp.draw.cpu().numpy().reshape(B, 16, 4), codes.cpu().numpy().reshape(B, 16, 4)
    for pos in range(16):
        for d in range(4):
            x = tc.kc.poisoned(logits.view(B, 16, 4, -1)[:, pos, d].contiguous())
            k = None if tc.ENGINE_TOP_K[d] >= 500 else tc.ENGINE_TOP_K[d]
            got = tc.call_trunc(nat, x, T=0.9, k=k, p=tc.ENGINE_TOP_P[d], min_p=tc.ENGINE_MIN_P[d], typ=tc.ENGINE_TYP[d], seed=tc.SEED,
                                offset=tc.OFFSET + pos * 4 + d, want_logp=True)
            assert np.array_equal(got.samples, cd[:, pos, d])
            tc.check_logp(draw[:, pos, d], got.probs, got.samples, f'position {pos} depth {d}')
            assert np.array_equal(got.logp.view(np.uint32), draw[:, pos, d].view(np.uint32))
    with ar.return_log_probs():
        codes1, lp1 = ar.sample(_zeros(), aux, cond=cond, temperature=0.9, min_p=1.0)
    d1 = lp1.draw.cpu().numpy()
    assert (d1 == 0.0).all() and not np.signbit(d1).any(), 'min_p = 1.0 leaves one token: its log-probability is +0.0'
    top = tc.masked_logits(ar, ar.teacher_forced_logits(codes1, aux, cond=cond)).argmax(dim=-1)
    assert torch.equal(top, codes1)


def test_engine_masks_and_guidance(nat, tiny):
    """kept codes stay and a truncated call's own codes replayed as `keep` return that call bit for bit; sample_guided at s = 1 equals
    sample over the 2B rows in its first half; one guided text-conditioned call draws only certified codes"""
    ar, aux, cond, uncond = tiny
    keep = M.replay_mask(B, 4, 4, 4, 7)
    M.check_replay(ar, aux, cond, keep, 5, **KW, **TR)
    G.check_s1_identity(ar, aux, _zeros(), cond, uncond, 5, **KW, **TR)
    G.check_s1_identity(ar, aux, _zeros(), cond, uncond, 5, keep_mask=torch.from_numpy(keep).to(DEV), **KW, **TR)
    out = ar.sample_guided(_zeros(), aux, cond=cond, uncond=uncond, guidance_scale=3.0, **KW, **TR)
    g = G.guided_step_logits(nat, ar, aux, out, cond, uncond, 3.0).cpu().numpy()
    n, tol = tc.engine_membership(nat, out.cpu().numpy(), g, 0.9, tc.ENGINE_TOP_K, tc.ENGINE_TOP_P, tc.ENGINE_MIN_P, tc.ENGINE_TYP,
                                  tc.SEED, tc.OFFSET, DEV, what='sample_guided')
    print(f'sample_guided: {n} codes certified, {tol} needed a boundary tolerance')
    assert tol <= 0.02 * n


def test_engine_guided_text(nat):
    """guided sampling of the text-conditioned fixture with both filters: graph == eager == cached=False"""
    ar, aux = M.model(C.RQT_TINY_TXT, 43, DEV)
    cond = M.cond_for(C.RQT_TINY_TXT, 2, DEV)
    uncond = G.uncond_for(C.RQT_TINY_TXT, cond)
    ar._draw_rng = lambda device, n: (tc.SEED, tc.OFFSET)
    (H, W, D) = ar.block_size
    zeros = torch.zeros((2, H, W, D), dtype=torch.long, device=DEV)
    kw = dict(temperature=0.9, top_k=50, min_p=0.05, typical_p=0.9, uncond=uncond, guidance_scale=2.0)
    a = ar.sample_guided(zeros, aux, cond=cond, **kw)
    ar.use_graph = False
    b = ar.sample_guided(zeros, aux, cond=cond, **kw)
    ar.use_graph = True
    assert torch.equal(a, b)
    assert torch.equal(a, ar.sample_guided(zeros, aux, cond=cond, cached=False, **kw))
    assert not torch.equal(a, ar.sample_guided(zeros, aux, cond=cond, **dict(kw, min_p=None, typical_p=None)))
