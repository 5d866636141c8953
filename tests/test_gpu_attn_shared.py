"""The shared-prompt decode attention alone on a real MI355X (`-m gpu`): rqamd_dbg_rqt_attn_shared (csrc/rqt_attn_shared.hip) against
rqamd_dbg_rqt_attn_decode on the expanded cache, bit for bit, over the full case list of tests/attn_shared_cases.py -- in the bf16 and the
fp16 build of the library -- and one case per form against fp64.
tests/test_emu_attn_shared.py runs a rotation of the same cases through the host emulator."""
import pytest
import torch

import attn_shared_cases as S

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    _native.lib16()
    return _native


@pytest.mark.parametrize('half', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('Ps', S.PS)
def test_gpu_shared_equals_plain_on_expanded_cache(nat, Ps, half):
    assert S.exact_cases(nat, DEV, Ps, half=half) == len(S.FANS) * len(S.HEADS) * len(S.TCAPS)


@pytest.mark.parametrize('which', ['small', 'reg'])
def test_gpu_shared_fp64(nat, which):
    print('shared %s, observed c %.3f' % (which, S.fp64_case(nat, DEV, which)))


def test_gpu_shared_refusals(nat):
    S.refusals(nat, DEV, pytest)
