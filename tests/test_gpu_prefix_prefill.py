"""The one-pass prefix prefill on the MI355X (`pytest -m gpu`): "prefix.one_pass", rqamd_rqt_step_prefill and
RQTransformer.prefix_mode = 'one_pass'.  The cases are tests/prefix_prefill_cases.py, shared with the emulator runs
(tests/test_emu_prefix_prefill.py); the long map, the fp16 build, the graphs and the time are checked here only."""
import statistics

import numpy as np
import pytest
import torch

from oracle import configs as C

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


# ---------------------------------------------------------------------------------------------- 1. logits after the prefill
@pytest.mark.parametrize('n0', PC.TINY_N0)
def test_prefill_logits_tiny(nat, golden, n0):
    PC.check_prefill_logits(PC.case(golden, 'tiny', DEV), n0, PC.REF_TINY, 'rqt_tiny')


@pytest.mark.parametrize('n0', PC.TXT_N0)
def test_prefill_logits_text_conditioned(nat, golden, n0):
    """4 conditioning tokens: the 3 text tokens of the prefix are part of the pass (3 + n0 tokens per image)"""
    PC.check_prefill_logits(PC.case(golden, 'txt', DEV), n0, PC.REF_TINY, 'rqt_tiny_txt')


@pytest.mark.parametrize('tag', sorted(PC.VARIANTS))
def test_prefill_logits_variants(nat, golden, tag):
    """tuple: learned token embeddings (body_input_kernel's table path); heads: head size 32 (the one-wavefront-per-token append);
    nocumsum"""
    PC.check_prefill_logits(PC.case(golden, tag, DEV), 9, PC.REF_TINY, f'variant {tag}')


# ---------------------------------------------------------------------------------------------- 2. chunking
def test_prefill_chunked(nat, golden):
    PC.check_chunked(PC.case(golden, 'tiny', DEV), PC.REF_TINY)


# ---------------------------------------------------------------------------------------------- 3. long contexts and cache formats
@pytest.mark.parametrize('n0', [1, 8, 15])
def test_prefill_long_text(nat, golden, n0):
    """rqt_long_txt300: 300 .. 314 tokens per image, text then codes, through the tiled append"""
    PC.check_prefill_logits(PC.case(golden, 'txt300', DEV), n0, PC.REF_LONG['gpu'], 'rqt_long_txt300')


@pytest.mark.parametrize('n0', [192, 193, 200, 1016])
def test_prefill_long_map(nat, golden, n0):
    """rqt_long_map, 32 x 32 behind 64 text tokens, 2 images: 63 + n0 tokens per image -- 255 (the plain kernel's longest), 256 (the tiled
    kernel's first), 263, and 1079 tokens with only the last eight positions stepped; every stored position >= n0 is compared"""
    PC.check_prefill_logits(PC.case(golden, 'map', DEV), n0, PC.REF_LONG['gpu'], 'rqt_long_map')


@pytest.mark.parametrize('fmt', ['int8k', 'int8kv'])
def test_prefill_int8_cache(nat, golden, monkeypatch, fmt):
    monkeypatch.setenv('RQAMD_KV', fmt)
    PC.check_prefill_logits(PC.case(golden, 'tiny', DEV), 9, PC.REF_INT8['gpu'], f'rqt_tiny, {fmt} cache')


def test_prefill_amp(nat, golden):
    """amp=True: the fp16 build of the engine"""
    PC.check_prefill_logits(PC.case(golden, 'tiny', DEV, amp=True), 9, PC.REF_F16, 'rqt_tiny, fp16 engine')


# ---------------------------------------------------------------------------------------------- 4.-9. the sampling forms
def test_forms_agree_and_draws_see_the_prefix(nat):
    ar, aux, cond, partial, codes, lp = PC.check_forms_agree(DEV)
    PC.check_conditioned_on_prefix(ar, aux, cond, partial, codes, lp)


def test_stale_cache(nat):
    PC.check_stale_cache(DEV)


def test_graphs_are_shared(nat):
    PC.check_graphs(DEV)


def test_errors(nat):
    PC.check_errors(nat, DEV)


def test_default_untouched(nat):
    PC.check_default_untouched(DEV)


def test_cached_forward_restart(nat):
    PC.check_cached_forward_restart(DEV)


# ---------------------------------------------------------------------------------------------- 10. time
def test_one_pass_prefix_is_faster(nat):
    """RQT_WIDE (the 1.4B layer shapes, 2 body layers + 1 head layer), 8 images, start_loc = (7, 7): the stepped call runs 63 eager body
    steps of 8 rows, the one-pass call one pass over 504 rows; both sample the last position.  The two modes alternate in one process,
    median of 5 each, device events.  Gate: the one-pass call takes at most a third of the stepped call (the gate of the one-pass
    forward at 8 images, tests/test_gpu_forward_onepass.py).  Measured on the MI355X: stepped 6.12 ms, one-pass 1.09 ms, 5.6x (DESIGN.md
    section 4c)."""
    cfg = C.RQT_WIDE
    ar, aux = M.model(cfg, 51, DEV)
    H, W, D = cfg['block_size']
    B = 8
    cond = M.cond_for(cfg, B, DEV)
    partial = PC.T(np.random.default_rng(7).integers(0, cfg['vocab_size'], (B, H, W, D)), DEV, torch.long)
    start = (H - 1, W - 1)

    def call(mode):
        ar.prefix_mode = mode
        M.seed_all(5)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = ar.sample(partial, aux, cond=cond, start_loc=start, top_k=50, top_p=0.9)
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)
    outs = {m: call(m)[0] for m in ('stepped', 'one_pass')}            # warm-up: workspaces, the position's graph
    ms = {'stepped': [], 'one_pass': []}
    for _ in range(5):
        for m in ms:
            out, t = call(m)
            assert torch.equal(out, outs[m])
            ms[m].append(t)
    for m, out in outs.items():
        assert torch.equal(out.view(B, H * W, D)[:, :-1], partial.view(B, H * W, D)[:, :-1]), m
    st, op = statistics.median(ms['stepped']), statistics.median(ms['one_pass'])
    print('prefix prefill, RQT_WIDE, 8 images, start_loc (7, 7): stepped %.3f ms, one-pass %.3f ms, ratio %.1fx' % (st, op, st / op))
    assert op * 3 <= st
