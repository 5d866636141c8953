"""CPU-only checks of anchored sampling (RQTransformer.anchor / rqamd_rqt_sample_anchor / rqamd_anchor_logits) through the host emulator
(tests/emu): the same .hip sources executed by fibers.  Apart from the fold against fp64 every comparison is exact.  The authoritative
runs, with captured graphs, the fp16 engine, the (257, 16384, 256) shape and the graph keys, are the `-m gpu` ones
(tests/test_gpu_anchored_sampling.py).  The emulator needs minutes for a full sampling pass, so the calls here carry the keep_mask of the
guided tests, which leaves three positions to run, or a mask with two steps to draw where the host loop runs."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchored_sampling_cases as A  # noqa: E402
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402

from oracle import configs as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
DEV = torch.device('cpu')
B = 3


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
    """the tiny model (4x4x4, V 500, dim 64) with the quantiser of the soft-loss fixture, 3 images"""
    ar, aux, cond, z = A.setup(DEV, B)
    ar.use_graph = False                                  # (the emulator has no stream capture)
    return ar, aux, cond, z


def _codes(seed=3):
    return G.random_codes((B, 4, 4, 4), 500, seed, DEV)


def _two_steps():
    """keep all but position 6, depth 0 (rows 0 and 2 only: the residual of row 1 follows a kept code) and depth 1 (every row): the host
    loop runs one teacher-forced pass of the whole map per step"""
    keep = torch.ones((B, 4, 4, 4), dtype=torch.bool)
    keep[:, 1, 2, :2] = False
    keep[1, 1, 2, 0] = True
    return keep


# ---------------------------------------------------------------------------------------------- 1. anchor_logits alone
@pytest.mark.parametrize('shape', [(1, 499, 64), (3, 500, 64), (5, 500, 128)])
@pytest.mark.parametrize('d', [0, 3])
def test_emu_anchor_logits(nat, shape, d):
    A.check_anchor_logits(nat, *shape, d, DEV, seed=shape[1] + d)


# ---------------------------------------------------------------------------------------------- 2. zero weight is the plain call
@pytest.mark.parametrize('sampler', sorted(M.SAMPLERS))
def test_emu_anchor_zero_weight_samplers(nat, tiny, sampler):
    ar, aux, cond, z = tiny
    keep = G.few_mask(B)
    A.check_zero_weight(ar, z, lambda: ar.sample(_codes(), aux, cond=cond, keep_mask=keep, **M.SAMPLERS[sampler]), seed=5)


def test_emu_anchor_zero_weight_forms(nat, tiny):
    ar, aux, cond, z = tiny
    keep = G.few_mask(B)
    uncond = G.uncond_for(C.RQT_TINY, cond)
    A.check_zero_weight(ar, z, lambda: ar.sample_guided(_codes(), aux, cond=cond, uncond=uncond, guidance_scale=3.0, top_k=50, keep_mask=keep), seed=6,
                        weight=torch.zeros((B, 4, 4, 4)))

    def per_image():
        with ar.seeds([11, 12, 13]):
            return ar.sample(_codes(), aux, cond=cond, temperature=torch.tensor([0.8, 1.0, 1.3]), top_k=torch.tensor([50, 500, 20]), keep_mask=keep)
    A.check_zero_weight(ar, z, per_image, seed=7, weight=[0.0] * 4)

    def logp():
        with ar.return_log_probs():
            return ar.sample(_codes(), aux, cond=cond, top_k=50, top_p=0.9, keep_mask=keep)
    A.check_zero_weight(ar, z, logp, seed=8)


# ---------------------------------------------------------------------------------------------- 3. engine == host loop
HOST_LOOP = {
    'per_depth_plain': (A.PER_DEPTH, dict()),
    'image_table_topk_topp_min_p': ('table', dict(top_k=50, top_p=0.9, min_p=0.05)),
}


@pytest.mark.parametrize('case', sorted(HOST_LOOP))
def test_emu_anchor_engine_equals_host_loop(nat, tiny, case):
    ar, aux, cond, z = tiny
    weight, kw = HOST_LOOP[case]
    weight = A.image_table(B) if weight == 'table' else weight
    keep = _two_steps()
    partial = torch.where(keep, _codes(5), torch.full((), M.OUT_OF_RANGE, dtype=torch.long))
    got = A.check_host_loop(ar, z, weight, lambda cached: ar.sample(partial, aux, cond=cond, keep_mask=keep, cached=cached, **kw), seed=7)
    assert torch.equal(got[keep], partial[keep])


def test_emu_anchor_guided_scheduled_host_loop(nat, tiny):
    """a guided call inside schedule(): the scheduled samplers and the scheduled host loop, both twins folded"""
    ar, aux, cond, z = tiny
    keep = _two_steps()
    partial = torch.where(keep, _codes(5), torch.full((), M.OUT_OF_RANGE, dtype=torch.long))
    uncond = G.uncond_for(C.RQT_TINY, cond)

    def scheduled(cached):
        with ar.schedule(temperature=ar.position_ramp(1.3, 0.7)):
            return ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=3.0, top_k=50, keep_mask=keep, cached=cached)
    A.check_host_loop(ar, z, 2.0, scheduled, seed=9)


def test_emu_anchor_changes_the_codes_and_follows_kept_codes(nat, tiny):
    """the residual follows the GIVEN code: with depth 0 kept at a code that is not the image's own, the anchored draw of depth 1 is the
    host loop's (which reads the kept code), and the anchor changes what is drawn"""
    ar, aux, cond, z = tiny
    keep = torch.ones((B, 4, 4, 4), dtype=torch.bool)
    keep[:, 0, 1, 1:3] = False                             # position 1: depth 0 kept, depths 1 and 2 drawn
    partial = _codes(9)
    M.seed_all(3)
    plain = ar.sample(partial, aux, cond=cond, keep_mask=keep)
    A.check_host_loop(ar, z, 64.0, lambda cached: ar.sample(partial, aux, cond=cond, keep_mask=keep, cached=cached), seed=3, differs_from=plain)


def test_emu_anchor_log_probs(nat, tiny):
    ar, aux, cond, z = tiny
    A.check_log_probs(nat, ar, aux, _codes(7), cond, z, 2.0, torch.full((B, 4, 4, 4), 2.0), seeds=[21, 22, 23], keep_mask=G.few_mask(B))


# ---------------------------------------------------------------------------------------------- 4. a strong anchor returns the image's codes
def test_emu_strong_anchor_returns_the_image_codes(nat, tiny):
    ar, aux, cond, _ = tiny
    k, z = A.strong_anchor_inputs(aux, B, 17, DEV)
    A.check_strong_anchor(nat, ar, aux, cond, k, z, keep_mask=G.few_mask(B))


# ---------------------------------------------------------------------------------------------- 6. refusals and signatures
def test_emu_anchor_refusals(nat, tiny):
    ar, aux, cond, z = tiny
    partial = _codes()
    ones = torch.ones((B, 4, 4, 4), dtype=torch.bool)

    def usable():
        assert torch.equal(ar.sample(partial, aux, cond=cond, top_k=50, keep_mask=ones), partial)
    A.check_refusals(ar, aux, cond, z, partial, usable, keep_mask=ones)
    A.check_tuple_refused(DEV, z)
    import ctypes
    keep8 = G.few_mask(B).to(torch.uint8).contiguous()
    active = (ctypes.c_uint8 * 16)(1, 1, 1)                # few_mask draws at positions 0 .. 2 only
    A.check_abi_refusals(nat, ar, aux, cond, z, partial, keep8=keep8, active=active)
    usable()


def test_anchor_signatures():
    from rqvae.models.rqtransformer import RQTransformer
    p = inspect.signature(RQTransformer.sample).parameters
    assert list(p)[-1] == 'keep_mask'                      # the argument lists are as they were: anchor() is a context
    q = inspect.signature(RQTransformer.anchor).parameters
    assert list(q) == ['self', 'z', 'weight']
