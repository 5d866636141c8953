"""CPU-only checks of shared-prompt sampling (rqamd_rqt_sample_shared, RQTransformer.shared_cond) through the host emulator (tests/emu: the
same .hip sources executed by fibers): RQT_TINY_TXT, 2 prompts x 4 images.  The cases are tests/shared_cond_cases.py, shared with the
authoritative `-m gpu` runs (tests/test_gpu_shared_cond.py), which add the real widths, amp=True and the run across GEMM regimes."""
import os
import sys

import pytest

import shared_cond_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = [pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build'), pytest.mark.slow]
DEV = 'cpu'


@pytest.fixture(scope='module')
def nat():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'emu'))
    import build_emu
    path = build_emu.build()
    from rqvae import _native
    import emu_binding
    saved = emu_binding.install(_native, path)
    yield _native
    SC.forget()
    emu_binding.restore(_native, saved)


# Trimmed against the GPU file, because a sampling call of the tiny model takes the emulator about a minute: the forms run composed
# (shared_cond_cases.FORMS_COMPOSED: three calls that touch every form but amp=True, which needs the fp16 build), once each -- the
# emulator has no stream capture, so "graphs" and "eager" are one path here -- and the checks around them draw the last two positions
# only ('late': start_loc = (3, 2); the fourteen positions before run the body stack and its shared attention all the same).
@pytest.mark.parametrize('form', SC.FORMS_COMPOSED)
def test_emu_shared_equals_repeated_cond(nat, form):
    SC.check_form(SC.setup('tiny', DEV), form, graphs=(True,))


def test_emu_shared_fan_one(nat):
    SC.check_fan_one(SC.setup('tiny', DEV), 'late')


def test_emu_second_call_other_prompts_and_back_to_plain(nat):
    SC.check_second_call_and_back(SC.setup('tiny', DEV), 'late', graphs=False)


def test_emu_kv_bytes(nat):
    print('kv bytes shared %d, plain %d' % SC.check_memory(SC.setup('tiny', DEV)))


def test_emu_errors(nat, monkeypatch):
    SC.check_errors(nat, DEV, monkeypatch, pytest, 'late')
