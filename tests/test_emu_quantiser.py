"""The certificate checks of tests/quantiser_check.py on the host emulator (tests/emu): the same checker and case builders as the
`-m gpu` twin (tests/test_gpu_quantiser.py), on a subset small enough for fibers -- every dim, one to three ring steps (the ring only
partly primed, the `newer == 1` / `newer == 0` branches of the counted wait), K < 4 (the norm DMA reads the codebook), one split case
whose last split holds a single code, and the constructed ties -- in both LDS-DMA landing modes (tests/emu/README.md).  The emulator
does not model how different wavefronts' DMAs land relative to each other: only the MI355X checks the counted waits."""
import os
import sys

import pytest

import quantiser_check as qc

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


@pytest.fixture(params=['issue', 'late'])
def dma(request, monkeypatch):
    """RQ_EMU_DMA: a DMA lands at issue (the default: worst case for a stage refilled too early) or as late as the counted wait allows"""
    if request.param == 'late':
        monkeypatch.setenv('RQ_EMU_DMA', 'late')
    else:
        monkeypatch.delenv('RQ_EMU_DMA', raising=False)
    return request.param


@pytest.mark.parametrize('case', qc.EMU_CASES, ids=lambda c: c.name)
def test_emu_quantiser_certificate(nat, dma, case):
    qc.run_quantize_case(nat, case, 'cpu', other_form=case.split)


@pytest.mark.parametrize('case', qc.EMU_TIE_CASES, ids=lambda c: c.name)
def test_emu_quantiser_ties(nat, dma, case):
    qc.run_quantize_case(nat, case, 'cpu', other_form=case.split)


def test_emu_quantiser_distances_and_soft_codes(nat, dma):
    """rq_distances and rq_soft_codes on one ragged single-tile case: the emulator runs the kernel's own fp32 operation order, so the
    bounds measured on the reference side (C_CHAIN, KAPPA up to the hardware's v_exp_f32) are met before a GPU sees them"""
    qc.run_distance_case(nat, qc.DIST_CASES[0], 'cpu')
    qc.run_soft_case(nat, qc.SOFT_CASES[0], 'cpu')
