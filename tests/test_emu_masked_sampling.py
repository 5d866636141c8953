"""CPU-only checks of masked sampling (RQTransformer.sample(keep_mask=...) / rqamd_rqt_sample_masked) through the host emulator
(tests/emu): the same .hip sources executed by fibers.  Every comparison is exact.  The authoritative runs, with captured graphs, the
fp16 engine, real widths and long contexts, are the `-m gpu` ones (tests/test_gpu_masked_sampling.py).  A 16-position pass of the
tiny model takes the emulator most of a minute, so the masks here leave few positions to run where the property allows it."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import masked_sampling_cases as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
DEV = torch.device('cpu')


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
    """RQT_TINY (4x4x4, V 500) with seeded weights, 2 images"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    ar.use_graph = False                                  # (the emulator has no stream capture)
    return ar, aux, M.cond_for(C.RQT_TINY, 2, DEV)


def _random_codes(B, seed=3):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 500, (B, 4, 4, 4)))


# ---------------------------------------------------------------------------------------------- 1. keep everything
def test_emu_masked_keep_everything(nat, tiny):
    ar, aux, cond = tiny
    partial = _random_codes(2)
    out = ar.sample(partial, aux, cond=cond, top_k=50, top_p=0.9, keep_mask=torch.ones((4, 4), dtype=torch.bool))
    assert torch.equal(out, partial)
    # at the ABI, without the per-position activity: every position runs, every sampler workgroup returns at once
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    keep = torch.ones((2, 4, 4, 4), dtype=torch.uint8)
    out = eng.sample_masked(partial, keep, None, cond, cbs, 1.0, [50, 50, 500, 500], [0.9, 1.0, 0.9, 1.0], 11, 0, False)
    assert torch.equal(out, partial)                       # (top-k kernel + general kernel, general kernel alone, unfiltered kernel)


# ---------------------------------------------------------------------------------------------- 2. prefix mask == start_loc
def test_emu_masked_prefix_equals_start_loc(nat, tiny):
    ar, aux, cond = tiny
    partial = _random_codes(2)
    keep = torch.zeros((4, 4), dtype=torch.bool)
    keep.view(-1)[:1 * 4 + 2] = True                       # the raster prefix before (1, 2): not a row boundary
    M.seed_all(9)
    want = ar.sample(partial, aux, cond=cond, start_loc=(1, 2), top_k=50, top_p=0.9)
    M.seed_all(9)
    got = ar.sample(partial, aux, cond=cond, top_k=50, top_p=0.9, keep_mask=keep)
    assert torch.equal(got, want)
    assert torch.equal(got.view(2, 16, 4)[:, :6], partial.view(2, 16, 4)[:, :6]) and not torch.equal(got, partial)
    # (start_loc composed with a mask: tests/test_gpu_masked_sampling.py)


# ---------------------------------------------------------------------------------------------- 3. replay
@pytest.mark.parametrize('sampler', ['plain', 'topk_topp'])
def test_emu_masked_replay(nat, tiny, sampler):
    ar, aux, cond = tiny
    keep = M.replay_mask(2, 4, 4, 4, seed=21)
    M.check_replay(ar, aux, cond, keep, seed=13, fillers=(M.OUT_OF_RANGE,), **M.SAMPLERS[sampler])


# ---------------------------------------------------------------------------------------------- 6. greedy / support
@pytest.mark.parametrize('top_k', [1, 50])
def test_emu_masked_greedy_and_support(nat, tiny, top_k):
    ar, aux, cond = tiny
    keep_t = torch.from_numpy(M.replay_mask(2, 4, 4, 4, seed=22))
    partial = torch.where(keep_t, _random_codes(2, seed=4), torch.zeros((), dtype=torch.long))
    M.seed_all(3)
    out = ar.sample(partial, aux, cond=cond, top_k=top_k, keep_mask=keep_t)
    M.check_support(ar, aux, cond, out, keep_t, partial, top_k)


# ---------------------------------------------------------------------------------------------- 7. host paths
def test_emu_masked_host_paths(nat, tiny):
    ar, aux, cond = tiny
    # three codes to draw: the uncached loop runs one teacher-forced pass of the whole map for each
    keep_t = torch.ones((2, 4, 4, 4), dtype=torch.bool)
    keep_t[0, 0, 3, 1] = False                             # position 3, depth 1, row 0 only
    keep_t[:, 1, 2, :2] = False                            # position 6, depths 0 and 1, both rows
    partial = torch.where(keep_t, _random_codes(2, seed=5), torch.full((), M.OUT_OF_RANGE, dtype=torch.long))
    M.seed_all(7)
    a = ar.sample(partial, aux, cond=cond, top_k=50, top_p=0.9, keep_mask=keep_t)
    M.seed_all(7)
    b = ar.sample(partial, aux, cond=cond, top_k=50, top_p=0.9, keep_mask=keep_t, cached=False)
    assert torch.equal(a, b)                               # the cache changes nothing, masked as unmasked
    ar.sampler = 'torch'
    try:
        M.seed_all(7)
        t = ar.sample(partial, aux, cond=cond, top_k=50, keep_mask=keep_t)
    finally:
        ar.sampler = 'philox'
    M.check_support(ar, aux, cond, t, keep_t, partial, 50)


# ---------------------------------------------------------------------------------------------- 9. refusals
def test_emu_masked_refusals(nat, tiny):
    ar, aux, cond = tiny
    partial = _random_codes(2)
    ones = torch.ones((2, 4, 4, 4), dtype=torch.bool)

    def usable():
        out = ar.sample(partial, aux, cond=cond, top_k=50, keep_mask=ones)
        assert torch.equal(out, partial)
    with pytest.raises(ValueError, match='shape'):
        ar.sample(partial, aux, cond=cond, keep_mask=torch.ones((4, 5), dtype=torch.bool))
    usable()
    with pytest.raises(ValueError, match='shape'):
        ar.sample(partial, aux, cond=cond, keep_mask=torch.ones((3, 4, 4, 4), dtype=torch.bool))
    with pytest.raises(ValueError, match='dtype'):
        ar.sample(partial, aux, cond=cond, keep_mask=torch.ones((4, 4), dtype=torch.float32))
    usable()
    bad = partial.clone()
    bad[1, 2, 3, 1] = 500                                  # vocab_size: one past the last code
    with pytest.raises(ValueError, match='vocab_size'):
        ar.sample(bad, aux, cond=cond, keep_mask=ones)
    usable()
    not_kept = ones.clone()
    not_kept[1, 2, 3, 1] = False                           # the same value where the code is drawn: not looked at
    out = ar.sample(bad, aux, cond=cond, top_k=50, keep_mask=not_kept)
    assert 0 <= int(out[1, 2, 3, 1]) < 500
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    with pytest.raises(ValueError, match='null'):          # RQAMD_ERR_INVALID
        eng.sample_masked(partial, None, None, cond, cbs, 1.0, [50] * 4, [1.0] * 4, 1, 0, False)
    usable()


def test_keep_mask_is_keyword_only():
    import inspect
    from rqvae.models.rqtransformer import RQTransformer
    p = inspect.signature(RQTransformer.sample).parameters
    assert p['keep_mask'].kind is inspect.Parameter.KEYWORD_ONLY and p['keep_mask'].default is None
    assert list(p)[-2:] == ['fast', 'keep_mask']           # the reference's arguments, then ours
