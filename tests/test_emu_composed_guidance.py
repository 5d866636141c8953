"""CPU-only checks of composed guidance (RQTransformer.extra_conds / rqamd_rqt_sample_compose / rqamd_compose_logits) through the host
emulator (tests/emu): the same .hip sources executed by fibers.  Apart from compose_logits against fp64 every comparison is exact.  The
authoritative runs, with captured graphs, the fp16 engine, real widths and the graph keys, are the `-m gpu` ones
(tests/test_gpu_composed_guidance.py).  A composed call runs (2 + K) B rows, so the calls here carry the keep_mask of the guided tests,
which leaves three positions to run."""
import inspect
import os
import sys

import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composed_guidance_cases as X  # noqa: E402
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
DEV = torch.device('cpu')
B = 2
WEIGHTS2 = (-1.5, 0.75)


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
    """RQT_TINY (4x4x4, V 500) with seeded weights, 2 images, cond, uncond and two extra conditionings that all differ in every row"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    ar.use_graph = False                                  # (the emulator has no stream capture)
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond), X.extras_for(C.RQT_TINY, cond, 2)


def _codes(seed=3):
    return G.random_codes((B, 4, 4, 4), 500, seed, DEV)


# ---------------------------------------------------------------------------------------------- 1. compose_logits against fp64
@pytest.mark.parametrize('V', [500, 499, 7])
def test_emu_compose_logits_fp64(nat, V):
    X.check_compose_logits(nat, 3, V, DEV, seed=V)
    X.check_negative_zero(nat, DEV)


# ---------------------------------------------------------------------------------------------- 2. identity with zero weights
@pytest.mark.parametrize('K,sampler', [(1, 1), (2, 0), (2, 2)])
def test_emu_composed_zero_weight_identity(nat, tiny, K, sampler):
    ar, aux, cond, uncond, extras = tiny
    X.check_zero_weight_identity(ar, aux, _codes(), cond, uncond, extras[:K], seed=5, keep_mask=G.few_mask(B), **G.SAMPLERS[sampler])


# ---------------------------------------------------------------------------------------------- 3. pairing
def test_emu_composed_pairing(nat, tiny):
    ar, aux, cond, uncond, _ = tiny
    assert X.check_equal_rows_equal_logits(ar, aux, _codes(9), cond, uncond)
    X.check_pairing(ar, aux, _codes(), cond, uncond, seed=11, keep_mask=G.few_mask(B), top_k=50, top_p=0.9)


# ---------------------------------------------------------------------------------------------- 4. greedy == argmax of the composed logits
def test_emu_composed_greedy_is_argmax(nat, tiny):
    ar, aux, cond, uncond, extras = tiny
    keep = G.few_mask(B)
    M.seed_all(3)
    with ar.extra_conds(conds=extras, weights=list(WEIGHTS2)):
        xs = ar.sample_guided(_codes(4), aux, cond=cond, uncond=uncond, guidance_scale=2.5, top_k=1, keep_mask=keep)
    assert torch.equal(xs[keep], _codes(4)[keep])
    X.check_composed_support(nat, ar, aux, xs, cond, uncond, extras, WEIGHTS2, 2.5, 1, drawn=~keep)


# ---------------------------------------------------------------------------------------------- 5. cached == uncached
def test_emu_composed_host_path(nat, tiny):
    ar, aux, cond, uncond, extras = tiny
    # two steps to draw: the uncached loop runs one teacher-forced pass of the whole map over the 3B rows for each
    keep = torch.ones((B, 4, 4, 4), dtype=torch.bool)
    keep[0, 0, 3, 1] = False                               # position 3, depth 1, row 0 only
    keep[:, 1, 2, 0] = False                               # position 6, depth 0, both rows
    partial = torch.where(keep, _codes(5), torch.full((), M.OUT_OF_RANGE, dtype=torch.long))
    kw = dict(cond=cond, uncond=uncond, guidance_scale=3.0, keep_mask=keep, top_k=50, top_p=0.9, negative=extras[0], negative_scale=1.5)
    M.seed_all(7)
    a = ar.sample_guided(partial, aux, **kw)
    M.seed_all(7)
    b = ar.sample_guided(partial, aux, cached=False, **kw)
    assert torch.equal(a, b)
    assert torch.equal(a[keep], partial[keep])


# ---------------------------------------------------------------------------------------------- 7. composition with the other forms
def test_emu_composed_masked_replay(nat, tiny):
    ar, aux, cond, uncond, extras = tiny
    X.check_composed_replay(ar, aux, _codes(6), cond, uncond, extras[:1], [-1.5], 3.0, seed=13, mask_seed=21, first_keep=G.few_mask(B),
                            top_k=50, top_p=0.9)


def test_emu_composed_per_image_weights_and_log_probs(nat, tiny):
    ar, aux, cond, uncond, extras = tiny
    keep = G.few_mask(B)
    X.check_per_image_weights(ar, aux, _codes(7), cond, uncond, extras[0], [-2.0, 1.25], seeds=[11, 12], keep_mask=keep, top_k=50, top_p=0.9)
    X.check_log_probs(nat, ar, aux, _codes(7), cond, uncond, extras[:1], [-0.5], seeds=[21, 22], keep_mask=keep)


# ---------------------------------------------------------------------------------------------- 8. refusals and signatures
def test_emu_composed_refusals(nat, tiny):
    ar, aux, cond, uncond, extras = tiny
    partial = _codes()
    ones = torch.ones((B, 4, 4, 4), dtype=torch.bool)
    kw = dict(cond=cond, uncond=uncond, guidance_scale=2.0, top_k=50, keep_mask=ones)

    def usable():
        assert torch.equal(ar.sample(partial, aux, cond=cond, top_k=50, keep_mask=ones), partial)
        assert torch.equal(ar.sample_guided(partial, aux, **kw), partial)
    five = [(cond + 1 + k) % 10 for k in range(5)]
    with pytest.raises(ValueError, match='extra conditions'):
        with ar.extra_conds(conds=five, weights=[0.5] * 5):
            ar.sample_guided(partial, aux, **kw)
    with pytest.raises(ValueError, match='finite'):
        with ar.extra_conds(conds=extras[:1], weights=[float('nan')]):
            ar.sample_guided(partial, aux, **kw)
    with pytest.raises(ValueError, match='weights'):
        with ar.extra_conds(conds=extras, weights=[0.5]):
            ar.sample_guided(partial, aux, **kw)
    usable()
    with pytest.raises(ValueError, match='shape'):
        with ar.extra_conds(conds=[torch.zeros((B + 1, 1), dtype=torch.long)], weights=[0.5]):
            ar.sample_guided(partial, aux, **kw)
    with pytest.raises(ValueError, match='shape'):
        with ar.extra_conds(conds=extras[:1], weights=[torch.zeros(B + 1)]):
            ar.sample_guided(partial, aux, **kw)
    usable()
    with pytest.raises(NotImplementedError, match='sample_guided'):
        with ar.extra_conds(conds=extras[:1], weights=[0.5]):
            ar.sample(partial, aux, cond=cond, top_k=50, keep_mask=ones)
    with pytest.raises(NotImplementedError, match='shared_cond'):
        with ar.shared_cond(1), ar.extra_conds(conds=extras[:1], weights=[0.5]):
            ar.sample_guided(partial, aux, **kw)
    with pytest.raises(ValueError, match='negative'):
        with ar.extra_conds(conds=extras[:1], weights=[0.5]):
            ar.sample_guided(partial, aux, negative=extras[1], **kw)
    ar.sampler = 'torch'
    try:
        with pytest.raises(NotImplementedError, match='torch'):
            ar.sample_guided(partial, aux, negative=extras[1], **kw)
    finally:
        ar.sampler = 'philox'
    usable()
    # at the ABI: K = 5 is refused when the call arms; a NaN weight, an unguided call and a shared-prompt arming when the armed call is made,
    # before anything is enqueued -- and each consumes the arming
    import ctypes
    from rqvae._native import _int_array, _ptr_array, ptr
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    L, h = eng._L, eng._h
    D = 4
    cb, tk, tp = _ptr_array(cbs[:D]), _int_array([50] * D), (ctypes.c_float * D)(*[1.0] * D)
    out = torch.empty_like(partial)
    keep8 = G.few_mask(B).to(torch.uint8).contiguous()
    active = (ctypes.c_uint8 * 16)(1, 1, 1)                # few_mask draws at positions 0 .. 2 only
    ex = (ctypes.c_void_p * 5)(*[ptr(e).value for e in five])
    w_ok, w_nan = (ctypes.c_float * (5 * B))(*[0.5] * (5 * B)), (ctypes.c_float * B)(0.5, float('nan'))

    def guided_call():
        return L.rqamd_rqt_sample_guided(h, ptr(partial), ptr(keep8), active, ptr(cond), ptr(uncond), B, cb, 0, 0, 1.0, 2.0, tk, tp, 2, 0, 0, ptr(out), None)
    assert guided_call() == 0
    ref = out.clone()
    assert L.rqamd_rqt_sample_compose(h, 5, ex, w_ok) == -1 and b'extra conditions' in L.rqamd_last_error()
    assert L.rqamd_rqt_sample_compose(h, 1, ex, w_nan) == 0
    assert guided_call() == -1 and b'finite' in L.rqamd_last_error()
    assert guided_call() == 0 and torch.equal(out, ref)    # (the refused call consumed the arming)
    assert L.rqamd_rqt_sample_compose(h, 1, ex, w_ok) == 0
    assert L.rqamd_rqt_sample_masked(h, ptr(partial), ptr(keep8), active, ptr(cond), B, cb, 1.0, tk, tp, 2, 0, 0, ptr(out), None) == -1
    assert b'unguided' in L.rqamd_last_error()
    assert L.rqamd_rqt_sample_compose(h, 1, ex, w_ok) == 0 and L.rqamd_rqt_sample_shared(h, 1) == 0
    assert guided_call() == -2 and b'rqamd_rqt_sample_shared' in L.rqamd_last_error()
    assert L.rqamd_rqt_sample_compose(h, 1, ex, w_ok) == 0 and L.rqamd_rqt_sample_compose(h, 0, None, None) == 0      # disarmed
    assert guided_call() == 0 and torch.equal(out, ref)
    # a NULL entry of extra_cond is zeros, as a NULL cond is
    nul = (ctypes.c_void_p * 1)(None)
    zero_cond = torch.zeros_like(cond)
    zer = (ctypes.c_void_p * 1)(ptr(zero_cond).value)
    res = []
    for arr in (nul, zer):
        assert L.rqamd_rqt_sample_compose(h, 1, arr, w_ok) == 0 and guided_call() == 0
        res.append(out.clone())
    assert torch.equal(res[0], res[1])
    usable()


def test_composed_signatures():
    from rqvae.models.rqtransformer import RQTransformer
    p = inspect.signature(RQTransformer.sample_guided).parameters
    assert list(p)[-3:] == ['uncond', 'guidance_scale', 'keep_mask']      # the argument list is as it was: negative= is a wrapper's keyword
    q = inspect.signature(RQTransformer.extra_conds).parameters
    assert list(q) == ['self', 'conds', 'weights']
    assert RQTransformer.MAX_EXTRA_CONDS == 4
