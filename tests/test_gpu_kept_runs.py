"""The one-pass fill of interior kept runs on the MI355X (`pytest -m gpu`): "masked.run_prefill", rqamd_rqt_step_run and
RQTransformer.kept_run_mode = 'one_pass'.  The cases are tests/kept_runs_cases.py, shared with the emulator runs
(tests/test_emu_kept_runs.py); the long map, the fp16 build and the time are checked here only."""
import statistics

import numpy as np
import pytest
import torch

from oracle import configs as C

import kept_runs_cases as K
import masked_sampling_cases as M
import prefix_prefill_cases as PC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    yield _native
    PC.forget_cases()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 1. logits behind a run
@pytest.mark.parametrize('runs', K.tiny_runs(), ids=str)
def test_run_logits_tiny(nat, golden, runs):
    K.check_run_logits(PC.case(golden, 'tiny', DEV), runs, PC.REF_TINY, 'rqt_tiny')


@pytest.mark.parametrize('runs', K.tiny_runs(), ids=str)
def test_run_logits_text_conditioned(nat, golden, runs):
    """4 conditioning tokens: the run extends caches that hold 3 text rows in front of the positions"""
    K.check_run_logits(PC.case(golden, 'txt', DEV), runs, PC.REF_TINY, 'rqt_tiny_txt')


def test_run_logits_learned_embeddings(nat, golden):
    """rqt_var_tuple: body_input_kernel's table path in its run form"""
    K.check_run_logits(PC.case(golden, 'tuple', DEV), [(2, 9)], PC.REF_TINY, 'variant tuple')


def test_run_logits_long_text(nat, golden):
    K.check_run_logits(PC.case(golden, 'txt300', DEV), [(1, 4), (6, 15)], PC.REF_LONG['gpu'], 'rqt_long_txt300')


def test_run_logits_long_map(nat, golden):
    """rqt_long_map, 32 x 32 behind 64 text tokens, 2 images (position p is cache row 63 + p): the run (130, 200) writes rows 193 .. 262,
    across row 256 and a key-tile edge of the past; the run (202, 1016) of 814 tokens per image extends 265 rows to 1079.  Heads at 200,
    201, 1016, 1017 and the last position, all stored in the fixture.  (No stale pass first: 1024 eager steps; the map's cache holds the
    rows of the stepped pass PC.case has just run over the same codes -- a row the passes left alone would not be seen here, which
    the tiny fixtures cover.)"""
    K.check_run_logits(PC.case(golden, 'map', DEV), [(130, 200), (202, 1016)], PC.REF_LONG['gpu'], 'rqt_long_map', stale=False)


def test_run_logits_amp(nat, golden):
    """amp=True: the fp16 build of the engine and of the extend kernel"""
    K.check_run_logits(PC.case(golden, 'tiny', DEV, amp=True), [(1, 3), (5, 9)], PC.REF_F16, 'rqt_tiny, fp16 engine')


def test_run_chunked(nat, golden):
    K.check_chunked(PC.case(golden, 'tiny', DEV), PC.REF_TINY)


# ---------------------------------------------------------------------------------------------- 2. sampling inside the mode
@pytest.mark.parametrize('name', ['left', 'band', 'start'])
def test_forms_agree_and_draws_see_the_runs(nat, name):
    ar, aux, cond, codes, lp, given = K.check_forms_agree(DEV, name)
    K.check_draws_see_the_runs(ar, aux, cond, codes, lp, given)


# ---------------------------------------------------------------------------------------------- 3.-5.
def test_default_untouched(nat):
    K.check_default_untouched(DEV)


def test_fallback_int8kv(nat, monkeypatch):
    monkeypatch.setenv('RQAMD_KV', 'int8kv')
    K.check_fallback_model(DEV, C.RQT_TINY)


def test_fallback_head_size_32(nat):
    K.check_fallback_model(DEV, C.RQT_TINY_HEADS)


def test_fallback_shared_prompt(nat):
    K.check_fallback_shared(DEV)


def test_single_position_runs(nat):
    K.check_single_position_runs(DEV)


def test_errors(nat):
    K.check_errors(nat, DEV)


# ---------------------------------------------------------------------------------------------- 6. time
def test_one_pass_runs_are_not_slower(nat):
    """RQT_WIDE (the 1.4B layer shapes, 2 body layers + 1 head layer), 8 images, the left 7 of 8 columns kept: the stepped call runs 56
    eager body steps of 8 rows, the one-pass call position 0, the run [1, 7) and seven runs of 7 positions (56 rows each).  The two modes
    alternate in one process, median of 5 each, device events.  Gate: the one-pass call is not slower than the stepped call of the same
    build.  Measured on the MI355X: stepped 9.77 ms, one-pass 6.18 ms, 1.58x."""
    cfg = C.RQT_WIDE
    ar, aux = M.model(cfg, 51, DEV)
    H, W, D = cfg['block_size']
    B = 8
    cond = M.cond_for(cfg, B, DEV)
    partial = PC.T(np.random.default_rng(7).integers(0, cfg['vocab_size'], (B, H, W, D)), DEV, torch.long)
    mask = torch.zeros((H, W), dtype=torch.bool, device=DEV)
    mask[:, :W - 1] = True

    def call(mode):
        ar.kept_run_mode = mode
        M.seed_all(5)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = ar.sample(partial, aux, cond=cond, keep_mask=mask, top_k=50, top_p=0.9)
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)
    outs = {m: call(m)[0] for m in ('stepped', 'one_pass')}            # warm-up: workspaces, the position graphs
    ms = {'stepped': [], 'one_pass': []}
    for _ in range(5):
        for m in ms:
            out, t = call(m)
            assert torch.equal(out, outs[m])
            ms[m].append(t)
    for m, out in outs.items():
        assert torch.equal(out[:, :, :W - 1], partial[:, :, :W - 1]), m
    st, op = statistics.median(ms['stepped']), statistics.median(ms['one_pass'])
    print('kept runs, RQT_WIDE, 8 images, left 7 of 8 columns kept: stepped %.3f ms, one-pass %.3f ms, ratio %.2fx' % (st, op, st / op))
    assert op <= st
