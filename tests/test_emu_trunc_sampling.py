"""Min-p and locally typical sampling on the host emulator (tests/emu): the chain certificates of tests/trunc_sampling_cases.py, the
same checker, cases and tolerances as the `-m gpu` twin (tests/test_gpu_trunc_sampling.py), on the cases with V <= 1024 and at most 8
rows each -- the emulator's fibers take about a second per filtered row, so the rest is marked `slow`.  The emulator runs the kernels'
own fp32 operation order with the host's logf / expf: the register form (sample_topk_kernel + trunc_regs) and the general form
(sample_kernel + trunc_lds) of every case are certified stage by stage before any GPU time is spent."""
import os
import sys

import pytest

import trunc_sampling_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')


@pytest.fixture(scope='module')
def nat():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'emu'))
    import build_emu
    path = build_emu.build()
    from rqvae import _native
    import emu_binding
    saved = emu_binding.install(_native, path)
    yield _native
    emu_binding.restore(_native, saved)


def _run(nat, case):
    out = tc.run_case(nat, case, 'cpu', rows_cap=tc.EMU_ROWS)
    print(f'{case.name}: largest deficit {out["worst"]:.3g} u, runner-up inside the tolerance in {out["near"]} of {out["rows"]} rows, '
          f'{out["band"]} entries inside the min-p band, forms that keep other sets in {out["diff"]} rows')
    return out


@pytest.mark.parametrize('case', [c for c in tc.CASES if c.emu == 1], ids=lambda c: c.name)
def test_emu_trunc_case(nat, case):
    _run(nat, case)


@pytest.mark.slow
@pytest.mark.parametrize('case', [c for c in tc.CASES if c.emu == 2], ids=lambda c: c.name)
def test_emu_trunc_case_slow(nat, case):
    out = _run(nat, case)
    if case.name.startswith('cap_'):
        assert (out['flags'] == int(case.k > tc.sc.SMP_CAP)).all()


def test_emu_trunc_rows(nat):
    """the per-row form with one seed per row: on rows against the scalar call, off rows against rqamd_sample_logits_rows"""
    seeds = [3, 2 ** 40 + 5, 3, 0, 7, 2 ** 62, 1, 2 ** 63 + 11, 2 ** 32, 2 ** 32 - 1, 15, 17]
    tc.run_rows_case(nat, 500, 'cpu', seeds, 99, 2 ** 32 + 1, 'row seeds V500')


@pytest.mark.slow
def test_emu_trunc_rows_call_seed(nat):
    tc.run_rows_case(nat, 7, 'cpu', None, what='rows V7')
    tc.run_rows_case(nat, 500, 'cpu', None, what='rows V500')


def test_emu_trunc_guided(nat):
    case = next(c for c in tc.CASES if c.name == 'V500_k62_all')
    tc.run_guided_case(nat, case._replace(rows=4), 'cpu')


def test_emu_trunc_refusals(nat):
    tc.check_refusals(nat, 'cpu')


# ---------------------------------------------------------------------------------------------- engine level
# A 16-position pass of the tiny model takes the emulator most of a minute, so the engine calls here carry
# guided_sampling_cases.few_mask, which leaves three positions to run; captured graphs and the fp16 engine are the `-m gpu` ones.
B = 3


@pytest.fixture(scope='module')
def tiny(nat):
    import torch
    import guided_sampling_cases as G
    import masked_sampling_cases as M
    from oracle import configs as C
    dev = torch.device('cpu')
    ar, aux = M.model(C.RQT_TINY, 41, dev)
    ar.use_graph = False                                  # (the emulator has no stream capture)
    ar._draw_rng = lambda device, n: (tc.SEED, tc.OFFSET)
    cond = M.cond_for(C.RQT_TINY, B, dev)
    keep = G.few_mask(B)
    partial = torch.where(keep, G.random_codes((B, 4, 4, 4), 500, 3, dev), torch.zeros((B, 4, 4, 4), dtype=torch.long))
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond), keep, partial


def test_emu_engine_armed_call(nat, tiny):
    """off values are the plain call; an armed call keeps the kept codes and draws other ones"""
    import torch
    ar, aux, cond, _, keep, partial = tiny
    kw = dict(temperature=0.9, top_k=tc.ENGINE_TOP_K, top_p=tc.ENGINE_TOP_P, keep_mask=keep)
    plain = ar.sample(partial, aux, cond=cond, **kw)
    with ar.truncation(min_p=0.0, typical_p=1.0):
        assert torch.equal(ar.sample(partial, aux, cond=cond, **kw), plain)
    out = ar.sample(partial, aux, cond=cond, **kw, min_p=tc.ENGINE_MIN_P, typical_p=tc.ENGINE_TYP)
    assert torch.equal(out[keep], partial[keep]) and not torch.equal(out, plain)


@pytest.mark.slow
def test_emu_engine_membership_and_paths(nat, tiny):
    """off values are the plain call; every drawn code of an armed call passes the chain certificates on its own teacher-forced logits;
    cached=False and the per-image form with the same values return the same codes; armed log-probabilities leave the codes alone"""
    import torch
    ar, aux, cond, _, keep, partial = tiny
    kw = dict(temperature=0.9, top_k=tc.ENGINE_TOP_K, top_p=tc.ENGINE_TOP_P, keep_mask=keep)
    tr = dict(min_p=tc.ENGINE_MIN_P, typical_p=tc.ENGINE_TYP)
    plain = ar.sample(partial, aux, cond=cond, **kw)
    assert torch.equal(ar.sample(partial, aux, cond=cond, **kw, min_p=0.0, typical_p=1.0), plain)
    out = ar.sample(partial, aux, cond=cond, **kw, **tr)
    assert torch.equal(out[keep], partial[keep]) and not torch.equal(out, plain)
    logits = tc.masked_logits(ar, ar.teacher_forced_logits(out, aux, cond=cond)).numpy()
    n, tol = tc.engine_membership(nat, out.numpy(), logits, 0.9, tc.ENGINE_TOP_K, tc.ENGINE_TOP_P, tc.ENGINE_MIN_P, tc.ENGINE_TYP, tc.SEED,
                                  tc.OFFSET, 'cpu', drawn=(~keep).numpy(), what='sample')
    print(f'sample: {n} codes certified, {tol} needed a boundary tolerance')
    assert n == int((~keep).sum()) and tol <= 1
    assert torch.equal(ar.sample(partial, aux, cond=cond, cached=False, **kw, **tr), out)
    with ar.return_log_probs():
        codes, lp = ar.sample(partial, aux, cond=cond, **kw, **tr)
    assert torch.equal(codes, out) and bool((lp.draw[keep] == 0).all()) and bool((lp.draw[~keep] <= 0).all())
    mp = torch.tensor([tc.ENGINE_MIN_P] * B)
    ty = torch.tensor([tc.ENGINE_TYP] * B)
    assert torch.equal(ar.sample(partial, aux, cond=cond, **kw, min_p=mp, typical_p=ty), out), 'the per-image form with equal values differs'


@pytest.mark.slow
def test_emu_engine_guided(nat, tiny):
    import torch
    import guided_sampling_cases as G
    ar, aux, cond, uncond, keep, partial = tiny
    kw = dict(temperature=0.9, top_k=tc.ENGINE_TOP_K, top_p=tc.ENGINE_TOP_P, min_p=tc.ENGINE_MIN_P, typical_p=tc.ENGINE_TYP)
    G.check_s1_identity(ar, aux, partial, cond, uncond, 5, keep_mask=keep, **kw)
    out = ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=3.0, keep_mask=keep, **kw)
    assert torch.equal(out, ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=3.0, keep_mask=keep, cached=False, **kw))


@pytest.mark.slow
def test_emu_abi_arming(nat, tiny):
    """rqamd_rqt_sample_trunc at the C ABI: consumed by a failing call, per-image arming refused in front of a scalar entry point,
    invalid values refused by the armed call, both NULL disarms"""
    import ctypes as C
    import torch
    ar, aux, cond, _, keep, partial = tiny
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    k8 = keep.to(torch.uint8).contiguous()
    pa = [bool(a) for a in (~keep).view(B, 16, 4).any(dim=2).any(dim=0).tolist()]
    call = lambda: eng.sample_masked(partial, k8, pa, cond, cbs, 0.9, tc.ENGINE_TOP_K, tc.ENGINE_TOP_P, tc.SEED, tc.OFFSET, False)
    plain = call()
    f4 = lambda v: (C.c_float * len(v))(*v)
    L = eng._L
    assert L.rqamd_rqt_sample_trunc(None, None, None, 0) == -1
    eng.arm_trunc(tc.ENGINE_MIN_P, tc.ENGINE_TYP)
    armed = call()
    assert not torch.equal(armed, plain) and torch.equal(call(), plain)                    # consumed by the call
    assert L.rqamd_rqt_sample_trunc(eng._h, f4(tc.ENGINE_MIN_P), None, 0) == 0
    assert L.rqamd_rqt_sample_trunc(eng._h, None, None, 0) == 0                            # both NULL disarms
    assert torch.equal(call(), plain)
    for mp, ty, per in ((f4([0.1] * 4 * B), None, 1), (f4([1.5, 0, 0, 0]), None, 0), (None, f4([float('nan')] * 4), 0)):
        assert L.rqamd_rqt_sample_trunc(eng._h, mp, ty, per) == 0
        with pytest.raises(ValueError):
            call()
        assert torch.equal(call(), plain)                                                  # consumed by the refused call
    eng.arm_trunc(tc.ENGINE_MIN_P, None)
    with pytest.raises(ValueError):                                                        # refused before sample_impl: still consumed
        eng.sample_masked(partial, k8, pa, cond, cbs, 0.0, tc.ENGINE_TOP_K, tc.ENGINE_TOP_P, tc.SEED, tc.OFFSET, False)
    assert torch.equal(call(), plain)


def test_signatures_and_exports():
    """min_p / typical_p are keywords of sample() and sample_guided() through a wrapper (their own argument lists stay as they were),
    truncation() is the context behind them, and the two new entry points are bound (rqamd_rqt_sample_trunc in the fp16 build too)"""
    import inspect
    from rqvae import _native
    from rqvae.models.rqtransformer import RQTransformer
    assert list(inspect.signature(RQTransformer.truncation).parameters) == ['self', 'min_p', 'typical_p']
    assert list(inspect.signature(RQTransformer.sample).parameters)[-1] == 'keep_mask'
    assert 'rqamd_rqt_sample_trunc' in _native.EXPORTS_F16 and 'rqamd_sample_logits_trunc' in _native.EXPORTS
    assert hasattr(_native.RqtEngine, 'arm_trunc') and callable(_native.sample_logits_trunc)
