"""CPU-only checks of the log-probabilities of the draws (rqamd_sample_logits_logp, rqamd_rqt_sample_logp,
RQTransformer.return_log_probs()) through the host emulator (tests/emu): the same .hip sources executed by fibers, with the host's expf /
logf.  The kernel-level checks are those of the GPU run, over the same matrices.  A 16-position pass of the tiny model takes the emulator
most of a minute, so the engine calls here carry guided_sampling_cases.few_mask, which leaves three positions to run; captured graphs, the
fp16 engine and the unmasked forms are the `-m gpu` ones (tests/test_gpu_sample_logp.py)."""
import inspect
import os
import sys

import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402
import sample_logp_cases as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
DEV = torch.device('cpu')
B = 3


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


@pytest.fixture(scope='module')
def tiny(nat):
    """RQT_TINY (4x4x4, V 500) with seeded weights, 3 images, cond and an uncond that differs from it in every row"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    ar.use_graph = False                                  # (the emulator has no stream capture)
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond)


# ---------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize('V', L.VOCABS)
def test_emu_logp_samples(nat, V):
    L.check_samples(nat, V, DEV)


@pytest.mark.parametrize('V', L.VOCABS)
def test_emu_logp_filtered_rows(nat, V):
    L.check_filtered(nat, V, DEV)


@pytest.mark.parametrize('V', L.VOCABS)
def test_emu_logp_unfiltered_rows(nat, V):
    L.check_unfiltered(nat, V, DEV)


@pytest.mark.parametrize('V', L.VOCABS)
def test_emu_logp_guided_rows(nat, V):
    L.check_guided(nat, V, DEV)


def test_emu_logp_refusals(nat):
    L.check_refusals(nat, DEV)


# ---------------------------------------------------------------------------------------------- engine level
@pytest.mark.parametrize('form', ['masked', 'per_image'])            # unguided scalar; guided per-image
def test_emu_engine_forms(nat, tiny, form):
    ar, aux, cond, uncond = tiny
    L.check_engine_form(nat, ar, aux, form, cond, uncond, few=True)


def test_emu_abi(nat, tiny):
    ar, aux, cond, uncond = tiny
    L.check_abi(nat, ar, aux, cond, uncond)


def test_emu_host_loops_refuse(nat, tiny):
    ar, aux, cond, uncond = tiny
    L.check_host_loops_refuse(ar, aux, cond, uncond)


def test_signatures():
    """return_log_probs() is a context, like seeds(): the argument lists of sample() and sample_guided() are as they were; the engine
    methods take want_logp=False last"""
    from rqvae import _native
    from rqvae.models.rqtransformer import RQTransformer, SampleLogProbs
    assert SampleLogProbs._fields == ('draw', 'model', 'model_uncond')
    assert list(inspect.signature(RQTransformer.sample).parameters)[-1] == 'keep_mask'
    assert list(inspect.signature(RQTransformer.return_log_probs).parameters) == ['self', 'on']
    for name in ('sample', 'sample_masked', 'sample_guided', 'sample_rows'):
        p = inspect.signature(getattr(_native.RqtEngine, name)).parameters
        assert list(p)[-1] == 'want_logp' and p['want_logp'].default is False
    assert 'rqamd_rqt_sample_logp' in _native.EXPORTS_F16 and 'rqamd_sample_logits_logp' in _native.EXPORTS
