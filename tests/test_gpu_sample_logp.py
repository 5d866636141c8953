"""Log-probabilities of the draws on the MI355X (`pytest -m gpu`): rqamd_sample_logits_logp over every LOGP build of the three sampler
kernels at real vocabulary sizes, rqamd_rqt_sample_logp through the four engine entry points with captured graphs on and off and on
both the bf16 and the fp16 engine, and RQTransformer.return_log_probs().  The checks live in tests/sample_logp_cases.py."""
import os
import sys

import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402
import sample_logp_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
B = 3


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


@pytest.fixture(scope='module')
def tiny(nat):
    """RQT_TINY (4x4x4, V 500) with seeded weights, 3 images, cond and an uncond that differs from it in every row"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond)


# ---------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize('V', L.VOCABS)
def test_logp_samples(nat, V):
    L.check_samples(nat, V, DEV)


@pytest.mark.parametrize('V', L.VOCABS)
def test_logp_filtered_rows(nat, V):
    L.check_filtered(nat, V, DEV)


@pytest.mark.parametrize('V', L.VOCABS)
def test_logp_unfiltered_rows(nat, V):
    L.check_unfiltered(nat, V, DEV)


@pytest.mark.parametrize('V', L.VOCABS)
def test_logp_guided_rows(nat, V):
    L.check_guided(nat, V, DEV)


def test_logp_refusals(nat):
    L.check_refusals(nat, DEV)


# ---------------------------------------------------------------------------------------------- engine level
@pytest.mark.parametrize('amp', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('form', L.FORMS)
def test_engine_forms(nat, tiny, form, graph, amp):
    """items 6 - 8: the codes of the armed call, the fill values, and draw / model / model_uncond re-derived from the engine's logits"""
    ar, aux, cond, uncond = tiny
    ar.use_graph = graph
    try:
        codes, lp = L.check_engine_form(nat, ar, aux, form, cond, uncond, amp=amp)
        if form == 'plain':
            L.check_sum_against_log_probs(ar, aux, codes, lp, cond, amp=amp)
    finally:
        ar.use_graph = True


@pytest.mark.parametrize('amp', [False, True], ids=['bf16', 'fp16'])
def test_graph_accounting(nat, amp):
    """the first armed call captures; a second one with other seeds captures nothing; an unarmed call in between neither captures nor
    invalidates; with graphs off the same codes and the same log-probabilities, bit for bit"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)                # a model of its own: no graph of an earlier test
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    uncond = G.uncond_for(C.RQT_TINY, cond)
    eng = ar._eng(amp)
    for form in ('plain', 'guided_masked', 'per_image_seeds'):
        plain0 = L.run_form(ar, aux, form, cond, uncond, False, amp)
        n_unarmed = eng.graph_captures()
        assert n_unarmed > 0
        a_codes, a_lp = L.run_form(ar, aux, form, cond, uncond, True, amp)
        n_armed = eng.graph_captures()
        assert n_armed > n_unarmed, (form, 'the first armed call captured nothing: it replayed graphs without the log-probability launches')
        b_codes, b_lp = L.run_form(ar, aux, form, cond, uncond, True, amp, seed=6)
        assert eng.graph_captures() == n_armed, (form, 'a second armed call captured again')
        plain1 = L.run_form(ar, aux, form, cond, uncond, False, amp)
        assert eng.graph_captures() == n_armed, (form, 'an unarmed call between armed ones captured')
        c_codes, c_lp = L.run_form(ar, aux, form, cond, uncond, True, amp)
        assert eng.graph_captures() == n_armed, (form, 'an unarmed call invalidated the armed graphs')
        assert torch.equal(plain0, plain1) and torch.equal(a_codes, plain0) and torch.equal(c_codes, a_codes)
        if form != 'per_image_seeds':
            assert not torch.equal(b_codes, a_codes)
        ar.use_graph = False
        try:
            e_codes, e_lp = L.run_form(ar, aux, form, cond, uncond, True, amp)
        finally:
            ar.use_graph = True
        assert eng.graph_captures() == n_armed
        assert torch.equal(e_codes, a_codes)
        for x, y, z in zip(a_lp, c_lp, e_lp):
            if x is not None:
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32)), form


@pytest.mark.parametrize('amp', [False, True], ids=['bf16', 'fp16'])
def test_abi(nat, tiny, amp):
    ar, aux, cond, uncond = tiny
    L.check_abi(nat, ar, aux, cond, uncond, amp)
    # through the binding: an armed call refused for a bad argument leaves the next call unarmed
    eng, cbs = ar._eng(amp), ar._checked_codebooks(aux)
    partial = torch.zeros((B, 4, 4, 4), dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match='temperature'):
        eng.sample(partial, cond, cbs, (0, 0), 0.0, [500] * 4, [1.0] * 4, 1, 0, False, want_logp=True)
    out = eng.sample(partial, cond, cbs, (0, 0), 1.0, [500] * 4, [1.0] * 4, 1, 0, False)
    assert torch.is_tensor(out)
    out2, lp = eng.sample(partial, cond, cbs, (0, 0), 1.0, [500] * 4, [1.0] * 4, 1, 0, False, want_logp=True)
    assert torch.equal(out, out2) and lp[2] is None and bool(torch.isfinite(lp[0]).all()) and bool(torch.isfinite(lp[1]).all())


def test_host_loops_refuse(tiny):
    ar, aux, cond, uncond = tiny
    L.check_host_loops_refuse(ar, aux, cond, uncond)
