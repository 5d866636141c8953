"""CPU-only checks of the soft-target cross entropy (rqamd_soft_ce, compute_loss(use_soft_target=True), rqamd_rqt_soft_loss /
RQTransformer.soft_target_loss) through the host emulator (tests/emu): the same .hip sources executed by fibers, against the fixture the
reference wrote (tests/golden/rqt_tiny_soft_loss.npz) and float64 of the reference's formula.  The cases live in
tests/soft_loss_cases.py; the authoritative runs are the `-m gpu` ones (tests/test_gpu_soft_loss.py)."""
import os
import sys

import pytest

import soft_loss_cases as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
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
    SL._SHARED.pop(DEV, None)                       # (engines of the emulator library: not to outlive its binding)
    emu_binding.restore(_native, saved)


@needs_clang
def test_emu_soft_ce_kernel_against_float64(nat):
    """case 1.  Largest |got - want| / max(1, |want|): 3.93e-07 here, 3.93e-07 on the MI355X (soft_loss_cases.KERNEL_MEASURED); the bound is
    twice the larger."""
    SL.check_kernel(nat, DEV, 'emu')


@needs_clang
def test_emu_soft_ce_kernel_nonfinite(nat):
    SL.check_kernel_nonfinite(nat, DEV)


@needs_clang
def test_emu_compute_loss_soft_target(nat, golden):
    SL.check_compute_loss(DEV, golden)


@needs_clang
def test_emu_soft_target_loss_targets_given(nat, golden):
    SL.check_form_a(DEV, golden)


@needs_clang
def test_emu_soft_target_loss_from_features(nat, golden):
    SL.check_form_b(DEV, golden, 'emu')


@needs_clang
def test_emu_soft_target_loss_onehot_is_log_probs(nat, golden):
    SL.check_onehot(DEV, golden, 'emu')


@needs_clang
@pytest.mark.slow
def test_emu_soft_target_loss_chunked(nat, golden):
    SL.check_chunked(DEV, golden, full=False)


@needs_clang
def test_emu_soft_target_loss_text_conditioned(nat, golden):
    SL.check_txt(DEV, golden)


@needs_clang
def test_emu_soft_target_loss_refusals(nat, golden):
    SL.check_refusals(nat, DEV, golden)
