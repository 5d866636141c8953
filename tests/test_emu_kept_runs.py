"""CPU-only checks of the one-pass fill of interior kept runs ("masked.run_prefill", rqamd_rqt_step_run, RQTransformer.kept_run_mode)
through the host emulator (tests/emu): the same .hip sources executed by fibers.  The cases are tests/kept_runs_cases.py, shared with the
authoritative `-m gpu` runs (tests/test_gpu_kept_runs.py); the long map, the fp16 build and the time are checked there only."""
import os
import sys

import pytest

from oracle import configs as C

import kept_runs_cases as K
import prefix_prefill_cases as PC

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
    PC.forget_cases()
    emu_binding.restore(_native, saved)


# ---------------------------------------------------------------------------------------------- 1. logits behind a run
@needs_clang
@pytest.mark.parametrize('runs', K.tiny_runs(), ids=str)
def test_emu_run_logits_tiny(nat, golden, runs):
    K.check_run_logits(PC.case(golden, 'tiny', DEV), runs, PC.REF_TINY, 'emu rqt_tiny')


@needs_clang
@pytest.mark.parametrize('runs', K.tiny_runs(), ids=str)
def test_emu_run_logits_text_conditioned(nat, golden, runs):
    """4 conditioning tokens: the run extends caches that hold 3 text rows in front of the positions"""
    K.check_run_logits(PC.case(golden, 'txt', DEV), runs, PC.REF_TINY, 'emu rqt_tiny_txt')


@needs_clang
def test_emu_run_logits_learned_embeddings(nat, golden):
    """rqt_var_tuple: body_input_kernel's table path in its run form"""
    K.check_run_logits(PC.case(golden, 'tuple', DEV), [(2, 9)], PC.REF_TINY, 'emu variant tuple')


@needs_clang
def test_emu_run_logits_long_text(nat, golden):
    """rqt_long_txt300: the runs extend caches of 300 and more rows (five and more key tiles of the past)"""
    K.check_run_logits(PC.case(golden, 'txt300', DEV), [(1, 4), (6, 15)], PC.REF_LONG['emu'], 'emu rqt_long_txt300')


@needs_clang
def test_emu_run_chunked(nat, golden):
    K.check_chunked(PC.case(golden, 'tiny', DEV), PC.REF_TINY)


# ---------------------------------------------------------------------------------------------- 2. sampling inside the mode
@needs_clang
@pytest.mark.parametrize('name', ['left', 'start'])
def test_emu_forms_agree_and_draws_see_the_runs(nat, name):
    """(the row-band mask runs on the GPU only: a dozen sampling calls through the emulator take minutes)"""
    ar, aux, cond, codes, lp, given = K.check_forms_agree(DEV, name)
    K.check_draws_see_the_runs(ar, aux, cond, codes, lp, given)


# ---------------------------------------------------------------------------------------------- 3.-5.
@needs_clang
def test_emu_default_untouched(nat):
    K.check_default_untouched(DEV)


@needs_clang
def test_emu_fallback_int8kv(nat, monkeypatch):
    monkeypatch.setenv('RQAMD_KV', 'int8kv')
    K.check_fallback_model(DEV, C.RQT_TINY)


@needs_clang
def test_emu_fallback_head_size_32(nat):
    K.check_fallback_model(DEV, C.RQT_TINY_HEADS)


@needs_clang
def test_emu_fallback_shared_prompt(nat):
    K.check_fallback_shared(DEV)


@needs_clang
def test_emu_single_position_runs(nat):
    K.check_single_position_runs(DEV)


@needs_clang
def test_emu_errors(nat):
    K.check_errors(nat, DEV)


def test_kept_run_mode_default_and_env(monkeypatch):
    from rqvae.models.rqtransformer import RQTransformer
    monkeypatch.delenv('RQAMD_KEPT_RUNS', raising=False)
    assert RQTransformer(C.RQT_TINY).kept_run_mode == 'stepped'
    monkeypatch.setenv('RQAMD_KEPT_RUNS', 'one_pass')
    assert RQTransformer(C.RQT_TINY).kept_run_mode == 'one_pass'
