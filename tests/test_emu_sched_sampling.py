"""Sampling schedules over positions and depths on the host emulator (tests/emu): the checks of tests/sched_sampling_cases.py that
the `-m gpu` twin (tests/test_gpu_sched_sampling.py) runs over whole maps, here over the three positions
guided_sampling_cases.few_mask leaves -- a 16-position pass of the tiny model takes the emulator most of a minute -- with everything
else kept.  The emulator runs the kernels' own index arithmetic, so the table index row * row_stride + pos * D + d of the scheduled
kernels, the host-side table fill and the arming are checked before any GPU time is spent; captured graphs and the fp16 engine are
the `-m gpu` ones.  The longer checks are marked `slow`."""
import os
import sys

import pytest

import sched_sampling_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
B = sc.B


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
    import torch
    import guided_sampling_cases as G
    import masked_sampling_cases as M
    from oracle import configs as C
    dev = torch.device('cpu')
    ar, aux = M.model(C.RQT_TINY, 41, dev)
    ar.use_graph = False                                  # (the emulator has no stream capture)
    sc.fix_rng(ar)
    cond = M.cond_for(C.RQT_TINY, B, dev)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond), G.few_mask(B)


def test_emu_constant_schedule(nat, tiny):
    """constant schedule == per-image call == scalar call: plain (masked) calls, the shared and the per-image table"""
    ar, aux, cond, _, keep = tiny
    sc.check_constant(ar, aux, cond, keep, shapes=('hw', 'bhwd'))


@pytest.mark.slow
def test_emu_constant_schedule_forms(nat, tiny):
    ar, aux, cond, uncond, keep = tiny
    sc.check_constant(ar, aux, cond, keep, shapes=('hwd',), trunc=True)
    sc.check_constant(ar, aux, cond, keep, uncond, shapes=('hw', 'bhwd'))
    sc.check_constant(ar, aux, cond, keep, seeds=[11, 2 ** 40 + 5, 11], shapes=('hwd',))


def test_emu_replay_every_index(nat, tiny):
    """the per-image table with the min-p / typical stages: every drawn (image, position, depth) replayed by the stand-alone sampler"""
    ar, aux, cond, _, keep = tiny
    sc.check_replay_every_index(nat, ar, aux, cond, True, True, keep)


@pytest.mark.slow
@pytest.mark.parametrize('per_image,trunc,guided', [(False, False, False), (False, True, True), (True, False, True)])
def test_emu_replay_every_index_forms(nat, tiny, per_image, trunc, guided):
    ar, aux, cond, uncond, keep = tiny
    sc.check_replay_every_index(nat, ar, aux, cond, per_image, trunc, keep, uncond if guided else None)


@pytest.mark.slow
def test_emu_uncached_and_own_replay(nat, tiny):
    """cached=False == the cached call; a scheduled call's own codes replayed as `keep` return that call"""
    import torch
    ar, aux, cond, _, keep = tiny
    sched = sc.distinct_schedule(True, True, False)
    with ar.schedule(**sched):
        a = sc.call(ar, aux, cond, keep)
        assert torch.equal(sc.call(ar, aux, cond, keep, cached=False), a), 'cached=False differs from the cached call'
        more = keep.clone()
        more[:, 0, 1, 1:] = True                              # keep some of what the call drew as well
        assert torch.equal(ar.sample(a, aux, cond=cond, keep_mask=more), a)


@pytest.mark.slow
def test_emu_effect(nat, tiny):
    """top-k 1 from position 2 on; guidance 1 -> 3 at position 2 (the seeds of sched_sampling_cases give codes that differ from
    both constant calls)"""
    ar, aux, cond, uncond, keep = tiny
    sc.check_greedy_from(ar, aux, cond, 2, keep)
    sc.check_guidance_halves(nat, ar, aux, cond, uncond, 2, keep)


def test_emu_refusals(nat, tiny):
    ar, aux, cond, uncond, keep = tiny
    # everything kept: a call that is not refused draws nothing, so the refusals are all this costs
    import torch
    all_kept = torch.ones_like(keep)
    sc.check_refusals(ar, aux, cond, uncond, all_kept)


@pytest.mark.slow
def test_emu_abi_arming(nat, tiny):
    ar, aux, cond, _, keep = tiny
    sc.check_c_refusals(nat, ar, aux, cond, keep)


def test_position_ramp_and_exports():
    """position_ramp; schedule() is a context with the six parameters as keywords, the argument lists of sample() / sample_guided()
    stay as they were, and the entry point is bound in both builds"""
    import inspect
    from oracle import configs as C
    from rqvae import _native
    from rqvae.models.rqtransformer import RQTransformer
    sc.check_position_ramp(RQTransformer(C.RQT_TINY))
    assert list(inspect.signature(RQTransformer.schedule).parameters) == ['self'] + list(sc.PARAMS)
    assert list(inspect.signature(RQTransformer.sample).parameters)[-1] == 'keep_mask'
    assert list(inspect.signature(RQTransformer.sample_guided).parameters)[-3:] == ['uncond', 'guidance_scale', 'keep_mask']
    assert 'rqamd_rqt_sample_schedule' in _native.EXPORTS_F16 and 'rqamd_rqt_sample_schedule' in _native.EXPORTS
    assert hasattr(_native.RqtEngine, 'arm_schedule')
