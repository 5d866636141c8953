"""Shared-prompt sampling on a real MI355X (`-m gpu`): rqamd_rqt_sample_shared / RQTransformer.shared_cond against the plain call with every
prompt repeated, bit for bit, on RQT_TINY_TXT (2 prompts x 4 images), RQT_TXT32 (2 x 2: 62 against 124 prefill rows) and RQT_TXT64 (1 x 2:
63 against 126) in every form of tests/shared_cond_cases.py -- the guided form, which doubles both prefills, on the sub-batches of
GUIDED_SHAPE there, for the reason given there -- and across GEMM regimes (RQT_TXT64, 3 x 43; guided at the full shapes of the two wide
fixtures) within the path-to-path bound.
tests/test_emu_shared_cond.py runs the tiny cases through the host emulator."""
import pytest
import torch

import shared_cond_cases as SC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    yield _native
    SC.forget()


@pytest.mark.parametrize('form', SC.FORMS)
@pytest.mark.parametrize('name', sorted(SC.SETUPS))
def test_gpu_shared_equals_repeated_cond(nat, name, form):
    s = SC.setup(name, DEV)
    SC.check_form(SC.guided_setup(s, name) if 'guided' in form else s, form)


@pytest.mark.parametrize('name', sorted(SC.SETUPS))
def test_gpu_shared_fan_one(nat, name):
    SC.check_fan_one(SC.setup(name, DEV))


@pytest.mark.parametrize('name', sorted(SC.SETUPS))
def test_gpu_second_call_other_prompts_and_back_to_plain(nat, name):
    SC.check_second_call_and_back(SC.setup(name, DEV))


@pytest.mark.parametrize('name', sorted(SC.SETUPS))
def test_gpu_kv_bytes(nat, name):
    print('kv bytes shared %d, plain %d' % SC.check_memory(SC.setup(name, DEV)))


def test_gpu_errors(nat, monkeypatch):
    SC.check_errors(nat, DEV, monkeypatch, pytest)


def test_gpu_shared_across_gemm_regimes(nat):
    SC.check_across_regimes(DEV)


@pytest.mark.parametrize('name', ['txt32', 'txt64'])
def test_gpu_guided_at_full_shape_across_gemm_regimes(nat, name):
    """guided, 2 x 2 on RQT_TXT32 and 1 x 2 on RQT_TXT64: the shapes at which the exact guided case cannot run (GUIDED_SHAPE)"""
    SC.check_guided_across_regimes(SC.setup(name, DEV))
