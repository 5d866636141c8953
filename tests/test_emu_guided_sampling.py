"""CPU-only checks of classifier-free guidance (RQTransformer.sample_guided / rqamd_rqt_sample_guided / rqamd_guide_logits) through the
host emulator (tests/emu): the same .hip sources executed by fibers.  Apart from guide_logits against fp64 every comparison is exact.
The authoritative runs, with captured graphs, the fp16 engine, real widths and the statistical test, are the `-m gpu` ones
(tests/test_gpu_guided_sampling.py).  A 16-position pass of the tiny model takes the emulator most of a minute and guidance doubles
the rows, so the calls here carry a keep_mask that leaves three positions to run wherever the property allows it."""
import inspect
import os
import sys

import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
DEV = torch.device('cpu')
B = 2


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
    """RQT_TINY (4x4x4, V 500) with seeded weights, 2 images, cond and an uncond that differs from it in every row"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    ar.use_graph = False                                  # (the emulator has no stream capture)
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond)


def _codes(seed=3):
    return G.random_codes((B, 4, 4, 4), 500, seed, DEV)


# ---------------------------------------------------------------------------------------------- 1. guide_logits against fp64
@pytest.mark.parametrize('V', [500, 499, 7])
def test_emu_guide_logits_fp64(nat, V):
    G.check_guide_logits(nat, 3, V, DEV, seed=V)


# ---------------------------------------------------------------------------------------------- 2. s = 1 identity
@pytest.mark.parametrize('sampler', range(len(G.SAMPLERS)))
def test_emu_guided_s1_identity(nat, tiny, sampler):
    ar, aux, cond, uncond = tiny
    assert bool((cond != uncond).all())
    G.check_s1_identity(ar, aux, _codes(), cond, uncond, seed=5, keep_mask=G.few_mask(B), **G.SAMPLERS[sampler])


# ---------------------------------------------------------------------------------------------- 3. greedy == argmax of the guided logits
def test_emu_guided_greedy_is_argmax(nat, tiny):
    ar, aux, cond, uncond = tiny
    keep = G.few_mask(B)
    M.seed_all(3)
    xs = ar.sample_guided(_codes(4), aux, cond=cond, uncond=uncond, guidance_scale=2.5, top_k=1, keep_mask=keep)
    assert torch.equal(xs[keep], _codes(4)[keep])
    G.check_guided_support(nat, ar, aux, xs, cond, uncond, 2.5, 1, drawn=~keep)


# ---------------------------------------------------------------------------------------------- 4. host paths
def test_emu_guided_host_paths(nat, tiny):
    ar, aux, cond, uncond = tiny
    # three codes to draw: the uncached loop runs one teacher-forced pass of the whole map over the 2B rows for each
    keep = torch.ones((B, 4, 4, 4), dtype=torch.bool)
    keep[0, 0, 3, 1] = False                               # position 3, depth 1, row 0 only
    keep[:, 1, 2, :2] = False                              # position 6, depths 0 and 1, both rows
    partial = torch.where(keep, _codes(5), torch.full((), M.OUT_OF_RANGE, dtype=torch.long))
    kw = dict(cond=cond, uncond=uncond, guidance_scale=3.0, keep_mask=keep)
    M.seed_all(7)
    a = ar.sample_guided(partial, aux, top_k=50, top_p=0.9, **kw)
    M.seed_all(7)
    b = ar.sample_guided(partial, aux, top_k=50, top_p=0.9, cached=False, **kw)
    assert torch.equal(a, b)                               # the cache changes nothing, guided as unguided
    assert torch.equal(a[keep], partial[keep])
    ar.sampler = 'torch'
    try:
        M.seed_all(7)
        t = ar.sample_guided(partial, aux, top_k=50, **kw)
    finally:
        ar.sampler = 'philox'
    assert torch.equal(t[keep], partial[keep])
    G.check_guided_support(nat, ar, aux, t, cond, uncond, 3.0, 50, drawn=~keep)


# ---------------------------------------------------------------------------------------------- 5. guided + masked replay
def test_emu_guided_masked_replay(nat, tiny):
    ar, aux, cond, uncond = tiny
    G.check_guided_replay(ar, aux, _codes(6), cond, uncond, 3.0, seed=13, mask_seed=21, first_keep=G.few_mask(B), top_k=50, top_p=0.9)


# ---------------------------------------------------------------------------------------------- 6. refusals and signatures
def test_emu_guided_refusals(nat, tiny):
    ar, aux, cond, uncond = tiny
    partial = _codes()
    ones = torch.ones((B, 4, 4, 4), dtype=torch.bool)

    def usable():
        out = ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=2.0, top_k=50, keep_mask=ones)
        assert torch.equal(out, partial)
    with pytest.raises(ValueError, match='shape'):
        ar.sample_guided(partial, aux, cond=cond, uncond=torch.zeros((B + 1, 1), dtype=torch.long), keep_mask=ones)
    usable()
    with pytest.raises(ValueError, match='shape'):
        ar.sample_guided(partial, aux, cond=cond, uncond=torch.zeros((B, 2), dtype=torch.long), keep_mask=ones)
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='finite'):
            ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=bad, keep_mask=ones)
        with pytest.raises(ValueError, match='finite'):
            nat.guide_logits(torch.zeros((2, 8)), torch.zeros((2, 8)), bad)
    usable()
    # at the ABI: a non-finite scale and a null `partial` are RQAMD_ERR_INVALID; a null `uncond` is zeros, as a null `cond` is
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    L, h = eng._L, eng._h
    D = 4
    from rqvae._native import _ptr_array, _int_array, ptr
    import ctypes
    cb, tk, tp = _ptr_array(cbs[:D]), _int_array([50] * D), (ctypes.c_float * D)(*[1.0] * D)
    out = torch.empty_like(partial)
    keep8 = G.few_mask(B).to(torch.uint8).contiguous()
    active = (ctypes.c_uint8 * 16)(1, 1, 1)                # few_mask draws at positions 0 .. 2 only

    def call(p, u, s, seed=1):
        return L.rqamd_rqt_sample_guided(h, p, ptr(keep8), active, ptr(cond), u, B, cb, 0, 0, 1.0, s, tk, tp, seed, 0, 0, ptr(out), None)
    assert call(None, ptr(uncond), 2.0) == -1 and b'null' in L.rqamd_last_error()
    assert call(ptr(partial), ptr(uncond), float('nan')) == -1 and b'finite' in L.rqamd_last_error()
    assert call(ptr(partial), ptr(uncond), float('inf')) == -1
    usable()
    assert call(ptr(partial), None, 2.0) == 0
    null_u = out.clone()
    zeros = torch.zeros_like(uncond)
    assert call(ptr(partial), ptr(zeros), 2.0) == 0
    assert torch.equal(out, null_u)
    usable()


def test_guided_signatures():
    from rqvae.models.rqtransformer import RQTransformer
    p = inspect.signature(RQTransformer.sample_guided).parameters
    for name, default in (('uncond', None), ('guidance_scale', 1.0), ('keep_mask', None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default
    assert list(p)[-3:] == ['uncond', 'guidance_scale', 'keep_mask']
    q = inspect.signature(RQTransformer.sample).parameters
    assert list(p)[:-3] == list(q)[:-1]                    # sample's arguments, in sample's order, then ours
    assert list(q)[-2:] == ['fast', 'keep_mask']           # sample itself is as it was
