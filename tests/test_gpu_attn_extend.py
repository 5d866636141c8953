"""The cache-extending causal attention alone on a real MI355X (`-m gpu`): rqamd_dbg_rqt_attn_extend (csrc/rqt_attn_extend.hip), bit for
bit against the prefill kernels over all T0 + R tokens and directly against fp64, with the cases, bound and side-effect checks of
tests/attn_extend_cases.py.  tests/test_emu_attn_extend.py runs the same cases through the host emulator."""
import pytest
import torch

import attn_extend_cases as X
import rqt_attn_cases as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


@pytest.mark.parametrize('kind', ['flat', 'peaked'])
@pytest.mark.parametrize('case', X.CASES, ids=X.case_id)
def test_gpu_extend_bit_identical_to_prefill(nat, case, kind):
    X.bit_identity(nat, DEV, case, kind)


@pytest.mark.parametrize('case', X.CASES_F16, ids=X.case_id)
def test_gpu_extend_bit_identical_to_prefill_fp16(nat, case):
    nat.lib16()
    X.bit_identity(nat, DEV, case, 'peaked', half=True)


@pytest.mark.parametrize('kind', X.KINDS)
@pytest.mark.parametrize('case', X.FP64_CASES, ids=X.case_id)
def test_gpu_extend_vs_fp64(nat, case, kind):
    c = X.fp64_check(nat, DEV, case, kind)
    print('gpu extend attention %s %s: observed c %.3f; so far: %s' % (X.case_id(case), kind, c, R.report()))


def test_gpu_extend_refusals(nat):
    X.refusals(nat, DEV, pytest)
