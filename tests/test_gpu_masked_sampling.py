"""Masked sampling on the MI355X (`pytest -m gpu`): RQTransformer.sample(keep_mask=...) over rqamd_rqt_sample_masked -- inpainting,
outpainting, depth refinement, a region per image.  Every comparison is exact: a code that is not kept is drawn from the logits, the
filter and the Philox counter of the unmasked call, so a masked call that is given what the unmasked call drew reproduces it bit for
bit; the stepped teacher-forced logits (RqtEngine.logits at the same batch) go through the kernels the sampling steps use."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import long_cases as L  # noqa: E402
import masked_sampling_cases as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


@pytest.fixture(scope='module')
def tiny(nat):
    """RQT_TINY (4x4x4, V 500) with seeded weights, 3 images"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    return ar, aux, M.cond_for(C.RQT_TINY, 3, DEV)


def _random_codes(B, seed=3):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 500, (B, 4, 4, 4))).to(DEV)


# ---------------------------------------------------------------------------------------------- 1. keep everything
def test_masked_keep_everything(tiny):
    ar, aux, cond = tiny
    partial = _random_codes(3)
    for mask in (torch.ones((3, 4, 4, 4), dtype=torch.bool, device=DEV), torch.ones((4, 4), dtype=torch.uint8)):
        out = ar.sample(partial, aux, cond=cond, top_k=50, top_p=0.9, keep_mask=mask)
        assert torch.equal(out, partial)
    # at the ABI, without the per-position activity: every position runs, every sampler workgroup returns at once
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    keep = torch.ones((3, 4, 4, 4), dtype=torch.uint8, device=DEV)
    for graph in (True, False):
        for top_k, top_p in (([50] * 4, [0.9] * 4), ([500] * 4, [1.0] * 4)):
            out = ar._on_side_stream(DEV, lambda: eng.sample_masked(partial, keep, None, cond, cbs, 1.0, top_k, top_p, 11, 0, graph))
            assert torch.equal(out, partial)


# ---------------------------------------------------------------------------------------------- 2. prefix mask == start_loc
@pytest.mark.parametrize('graph', [True, False])
def test_masked_prefix_equals_start_loc(tiny, graph):
    ar, aux, cond = tiny
    partial = _random_codes(3)
    keep = torch.zeros((4, 4), dtype=torch.bool, device=DEV)
    keep.view(-1)[:1 * 4 + 2] = True                       # the raster prefix before (1, 2): not a row boundary
    ar.use_graph = graph
    try:
        M.seed_all(9)
        want = ar.sample(partial, aux, cond=cond, start_loc=(1, 2), top_k=50, top_p=0.9)
        M.seed_all(9)
        got = ar.sample(partial, aux, cond=cond, top_k=50, top_p=0.9, keep_mask=keep)
        M.seed_all(9)                                      # start_loc composes with a mask: the positions before it are kept in addition
        both = ar.sample(partial, aux, cond=cond, start_loc=(1, 2), top_k=50, top_p=0.9, keep_mask=torch.zeros((3, 4, 4), dtype=torch.int32))
    finally:
        ar.use_graph = True
    assert torch.equal(got, want) and torch.equal(both, want)
    assert torch.equal(got.view(3, 16, 4)[:, :6], partial.view(3, 16, 4)[:, :6]) and not torch.equal(got, partial)


# ---------------------------------------------------------------------------------------------- 3. replay
REPLAY = {'b3': (C.RQT_TINY, {}), 'b3_large_batch_kernels': (C.RQT_TINY, {}), 'fp16_engine': (C.RQT_TINY, dict(amp=True)),
          'text_prefix': (C.RQT_TINY_TXT, {}), 'tuple_vocab': (C.RQT_TINY_TUPLE, {})}


@pytest.mark.parametrize('sampler', sorted(M.SAMPLERS))
@pytest.mark.parametrize('config', sorted(REPLAY))
def test_masked_replay(nat, tiny, config, sampler):
    cfg, kw = REPLAY[config]
    keep = M.replay_mask(3, 4, 4, 4, seed=21)
    if config == 'b3':
        ar, aux, cond = tiny
        M.check_replay(ar, aux, cond, keep, seed=13, **M.SAMPLERS[sampler], **kw)
        return
    # a model of its own: the kernel variants that dbg_set_row_scale selects are baked into captured graphs
    ar, aux = M.model(cfg, 41, DEV)
    cond = M.cond_for(cfg, 3, DEV)
    if config == 'b3_large_batch_kernels':
        nat.dbg_set_row_scale(4096)
    try:
        M.check_replay(ar, aux, cond, keep, seed=13, **M.SAMPLERS[sampler], **kw)
    finally:
        nat.dbg_set_row_scale(1)


# ---------------------------------------------------------------------------------------------- 4. real widths
def test_masked_replay_real_widths(nat):
    """E 1536, V 16384, 2 + 1 layers, 8x8x4, 5 images, top_k 1024 / top_p 0.95: the register top-k sampler at the product's vocabulary"""
    ar, aux = M.model(C.RQT_WIDE, 43, DEV)
    cond = M.cond_for(C.RQT_WIDE, 5, DEV)
    keep = M.replay_mask(5, 8, 8, 4, seed=24)
    M.check_replay(ar, aux, cond, keep, seed=17, top_k=1024, top_p=0.95)


# ---------------------------------------------------------------------------------------------- 5. long context
def test_masked_replay_long_context(nat):
    """context 315 (300 text tokens, 4x4x2 codes): the catch-all graph bucket and attn_long_kernel; odd positions kept"""
    cfg = L.txt_cfg(300)
    ar, aux = M.model(cfg, L.TXT300_SEED, DEV)
    cond = M.cond_for(cfg, 2, DEV)
    keep = np.zeros((2, 16, 2), dtype=bool)
    keep[:, 1::2] = True
    M.check_replay(ar, aux, cond, keep.reshape(2, 4, 4, 2), seed=19, top_k=50, top_p=0.9)


# ---------------------------------------------------------------------------------------------- 6. greedy / support
@pytest.mark.parametrize('top_k', [1, 50])
def test_masked_greedy_and_support(tiny, top_k):
    ar, aux, cond = tiny
    keep_t = torch.from_numpy(M.replay_mask(3, 4, 4, 4, seed=22)).to(DEV)
    partial = torch.where(keep_t, _random_codes(3, seed=4), torch.zeros((), dtype=torch.long, device=DEV))
    M.seed_all(3)
    out = ar.sample(partial, aux, cond=cond, top_k=top_k, keep_mask=keep_t)
    M.check_support(ar, aux, cond, out, keep_t, partial, top_k)


# ---------------------------------------------------------------------------------------------- 7. host paths
def test_masked_host_paths(tiny):
    ar, aux, cond = tiny
    cond = cond[:2].contiguous()
    keep_t = torch.from_numpy(M.replay_mask(2, 4, 4, 4, seed=23)).to(DEV)
    partial = torch.where(keep_t, _random_codes(2, seed=5), torch.full((), M.OUT_OF_RANGE, dtype=torch.long, device=DEV))
    for kw in (dict(top_k=50, top_p=0.9), dict()):
        M.seed_all(7)
        a = ar.sample(partial, aux, cond=cond, keep_mask=keep_t, **kw)
        M.seed_all(7)
        b = ar.sample(partial, aux, cond=cond, keep_mask=keep_t, cached=False, **kw)
        assert torch.equal(a, b), kw                       # the cache changes nothing, masked as unmasked
    ar.sampler = 'torch'
    try:
        M.seed_all(7)
        t = ar.sample(partial, aux, cond=cond, top_k=50, keep_mask=keep_t)
    finally:
        ar.sampler = 'philox'
    M.check_support(ar, aux, cond, t, keep_t, partial, 50)


# ---------------------------------------------------------------------------------------------- 8. graph hygiene
def test_masked_graph_hygiene(nat):
    """unmasked, masked, unmasked on one handle: the unmasked graphs are what they were, and what a handle that never saw a mask has"""
    kw = dict(top_k=50, top_p=0.9)
    zeros = torch.zeros((3, 4, 4, 4), dtype=torch.long, device=DEV)
    cond = M.cond_for(C.RQT_TINY, 3, DEV)
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    M.seed_all(31)
    u1 = ar.sample(zeros, aux, cond=cond, **kw)
    keep_t = torch.from_numpy(M.replay_mask(3, 4, 4, 4, seed=25)).to(DEV)
    m1 = ar.sample(_random_codes(3), aux, cond=cond, keep_mask=keep_t, **kw)
    M.seed_all(31)
    u2 = ar.sample(zeros, aux, cond=cond, **kw)
    m2 = ar.sample(_random_codes(3), aux, cond=cond, keep_mask=keep_t, **kw)      # (and back: the masked graphs are still there)
    assert torch.equal(m1[keep_t], m2[keep_t])
    fresh, aux2 = M.model(C.RQT_TINY, 41, DEV)
    M.seed_all(31)
    u3 = fresh.sample(zeros, aux2, cond=cond, **kw)
    assert torch.equal(u1, u2) and torch.equal(u1, u3)


# ---------------------------------------------------------------------------------------------- 9. refusals
def test_masked_refusals(tiny):
    ar, aux, cond = tiny
    partial = _random_codes(3)
    ones = torch.ones((3, 4, 4, 4), dtype=torch.bool, device=DEV)

    def usable():
        M.seed_all(1)
        a = ar.sample(partial, aux, cond=cond, top_k=50, keep_mask=ones[0, :, :, 0] & False)
        M.seed_all(1)
        b = ar.sample(partial, aux, cond=cond, top_k=50)
        assert torch.equal(a, b)                           # nothing kept: the unmasked call
    with pytest.raises(ValueError, match='shape'):
        ar.sample(partial, aux, cond=cond, keep_mask=torch.ones((4, 5), dtype=torch.bool, device=DEV))
    usable()
    with pytest.raises(ValueError, match='shape'):
        ar.sample(partial, aux, cond=cond, keep_mask=torch.ones((2, 4, 4, 4), dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match='dtype'):
        ar.sample(partial, aux, cond=cond, keep_mask=torch.ones((4, 4), dtype=torch.float32, device=DEV))
    usable()
    bad = partial.clone()
    bad[1, 2, 3, 1] = 500                                  # vocab_size: one past the last code
    with pytest.raises(ValueError, match='vocab_size'):
        ar.sample(bad, aux, cond=cond, keep_mask=ones)
    usable()
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    with pytest.raises(ValueError, match='null'):          # RQAMD_ERR_INVALID
        eng.sample_masked(partial, None, None, cond, cbs, 1.0, [50] * 4, [1.0] * 4, 1, 0, True)
    usable()
