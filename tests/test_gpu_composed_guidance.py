"""Composed guidance on the MI355X (`pytest -m gpu`): RQTransformer.extra_conds / sample_guided(negative=...) over
rqamd_rqt_sample_compose, and rqamd_compose_logits.  A composed call runs the engine over (2 + K) B rows; a fold launch per head step
writes c' and u' of every pair to a scratch, the guided sampler draws row b from guide(c'_b, u'_b, s) and writes the code to all K + 2
rows of the image.  Apart from compose_logits against fp64 every comparison is exact.  Captured graphs are on unless a test says
otherwise."""
import os
import sys

import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composed_guidance_cases as X  # noqa: E402
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


def _setup(cfg, B, K=2, seed=41):
    ar, aux = M.model(cfg, seed, DEV)
    cond = M.cond_for(cfg, B, DEV)
    uncond = G.uncond_for(cfg, cond)
    H, W, D = cfg['block_size']
    return ar, aux, cond, uncond, X.extras_for(cfg, cond, K), torch.zeros((B, H, W, D), dtype=torch.long, device=DEV)


@pytest.fixture(scope='module')
def tiny3(nat):
    """RQT_TINY (4x4x4, V 500) with seeded weights, 3 images, two extra conditionings"""
    return _setup(C.RQT_TINY, 3)


# ---------------------------------------------------------------------------------------------- 1. compose_logits against fp64
@pytest.mark.parametrize('shape', [(5, 16384), (3, 499)])
def test_compose_logits_fp64(nat, shape):
    X.check_compose_logits(nat, shape[0], shape[1], DEV, seed=shape[1])
    X.check_negative_zero(nat, DEV)


# ---------------------------------------------------------------------------------------------- 2. identity with zero weights
IDENTITY = {'b2': (C.RQT_TINY, 2, {}), 'b40': (C.RQT_TINY, 40, {}), 'text_prefix_b3': (C.RQT_TINY_TXT, 3, {}),
            'fp16_engine': (C.RQT_TINY, 2, dict(amp=True))}


@pytest.mark.parametrize('config', sorted(IDENTITY))
def test_composed_zero_weight_identity(nat, config):
    cfg, B, extra = IDENTITY[config]
    ar, aux, cond, uncond, extras, zeros = _setup(cfg, B)
    for K in (1, 2):
        for kw in G.SAMPLERS:
            X.check_zero_weight_identity(ar, aux, zeros, cond, uncond, extras[:K], seed=5, **kw, **extra)


# ---------------------------------------------------------------------------------------------- 3. pairing
def test_composed_pairing(tiny3):
    ar, aux, cond, uncond, _, zeros = tiny3
    xs = G.random_codes((3, 4, 4, 4), 500, 9, DEV)
    assert X.check_equal_rows_equal_logits(ar, aux, xs, cond, uncond), 'equal input rows of one launch gave different logits'
    X.check_pairing(ar, aux, zeros, cond, uncond, seed=11, top_k=50, top_p=0.9)


# ---------------------------------------------------------------------------------------------- 4. greedy == argmax / support
WEIGHTS2 = (-1.5, 0.75)


@pytest.fixture(scope='module')
def wide4(nat):
    """RQT_WIDE (E 1536, V 16384, 8x8x4), 4 images: the fold and the sampler rows at the product's width"""
    return _setup(C.RQT_WIDE, 4, seed=43)


def _greedy(nat, setup, top_k, top_p=None, seed=3):
    ar, aux, cond, uncond, extras, zeros = setup
    M.seed_all(seed)
    with ar.extra_conds(conds=extras, weights=list(WEIGHTS2)):
        xs = ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=2.5, top_k=top_k, top_p=top_p)
    X.check_composed_support(nat, ar, aux, xs, cond, uncond, extras, WEIGHTS2, 2.5, top_k)
    return xs


def test_composed_greedy_is_argmax_tiny(nat):
    setup = _setup(C.RQT_TINY, 4)
    xs = _greedy(nat, setup, 1)
    ar, aux, cond, uncond, extras, zeros = setup
    M.seed_all(3)                                          # and the extra conditions do change the greedy codes
    assert not torch.equal(xs, ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=2.5, top_k=1))


def test_composed_greedy_is_argmax_real_width(nat, wide4):
    _greedy(nat, wide4, 1)


def test_composed_support_real_width(nat, wide4):
    _greedy(nat, wide4, 1024, 0.95, seed=4)


# ---------------------------------------------------------------------------------------------- 5. graph == eager == uncached
def test_composed_graph_eager_uncached_agree(tiny3):
    ar, aux, cond, uncond, extras, zeros = tiny3
    kw = dict(cond=cond, uncond=uncond, guidance_scale=3.0, top_k=50, top_p=0.9, negative=extras[0], negative_scale=1.5)
    M.seed_all(7)
    a = ar.sample_guided(zeros, aux, **kw)
    ar.use_graph = False
    try:
        M.seed_all(7)
        b = ar.sample_guided(zeros, aux, **kw)
    finally:
        ar.use_graph = True
    M.seed_all(7)
    c = ar.sample_guided(zeros, aux, cached=False, **kw)
    assert torch.equal(a, b), 'captured graphs and eager launches differ'
    assert torch.equal(a, c), 'cached=True and cached=False differ'
    M.seed_all(7)                                          # negative= is sugar for the context with the weight negated
    with ar.extra_conds(conds=[extras[0]], weights=[-1.5]):
        assert torch.equal(a, ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=3.0, top_k=50, top_p=0.9))


# ---------------------------------------------------------------------------------------------- 6. graph keys
def test_composed_graph_keys(nat):
    """plain; composed K = 1; guided; composed K = 1 with another weight; composed K = 2; the first composed call again; plain again, on
    one handle: equal calls return equal codes, the two weights different ones, each call what a fresh handle returns, and the second
    K = 1 call captures nothing"""
    ar, aux, cond, uncond, extras, zeros = _setup(C.RQT_TINY, 3)
    kw = dict(top_k=50, top_p=0.9)
    gk = dict(cond=cond, uncond=uncond, guidance_scale=3.0, **kw)

    def plain(m, a):
        M.seed_all(1)
        return m.sample(zeros, a, cond=cond, **kw)

    def guided(m, a):
        M.seed_all(2)
        return m.sample_guided(zeros, a, **gk)

    def composed(m, a, K, w):
        M.seed_all(2)
        with m.extra_conds(conds=extras[:K], weights=[w] * K):
            return m.sample_guided(zeros, a, **gk)
    p1 = plain(ar, aux)
    c1a = composed(ar, aux, 1, -1.5)
    g1 = guided(ar, aux)
    eng = ar._eng(False)
    before = eng.graph_captures()
    c1w = composed(ar, aux, 1, 0.75)
    assert eng.graph_captures() == before, 'a new weight recaptured graphs'
    c2 = composed(ar, aux, 2, -1.5)
    assert eng.graph_captures() > before
    c1b = composed(ar, aux, 1, -1.5)
    p2 = plain(ar, aux)
    g2 = guided(ar, aux)
    # (the K = 2 call grew the workspace to 12 rows, which drops every graph once; from here on the handle is as large as it gets:)
    c2b = composed(ar, aux, 2, -1.5)                       # another K: the composed sets are recaptured ...
    mid = eng.graph_captures()
    p3, g3 = plain(ar, aux), guided(ar, aux)               # ... and nothing else is
    assert eng.graph_captures() == mid, 'plain or guided graphs were recaptured after a composed call with another K'
    assert torch.equal(p1, p3) and torch.equal(g1, g3) and torch.equal(c2, c2b)
    assert torch.equal(p1, p2) and torch.equal(g1, g2) and torch.equal(c1a, c1b)
    assert not torch.equal(c1a, c1w), 'two weights returned the same codes'
    assert not torch.equal(c1a, g1) and not torch.equal(c1a, c2)
    for call, want in ((lambda m, a: composed(m, a, 1, -1.5), c1a), (lambda m, a: composed(m, a, 1, 0.75), c1w),
                       (lambda m, a: composed(m, a, 2, -1.5), c2), (guided, g1), (plain, p1)):
        fresh, aux2 = M.model(C.RQT_TINY, 41, DEV)
        assert torch.equal(call(fresh, aux2), want)


# ---------------------------------------------------------------------------------------------- 7. composition with the other forms
@pytest.mark.parametrize('start_loc', [(0, 0), (1, 2)])
def test_composed_masked_replay(tiny3, start_loc):
    ar, aux, cond, uncond, extras, _ = tiny3
    partial = G.random_codes((3, 4, 4, 4), 500, 6, DEV)    # (the prefix before start_loc is given)
    codes0 = X.check_composed_replay(ar, aux, partial, cond, uncond, extras, [-1.5, 0.75], 3.0, seed=13, mask_seed=21, start_loc=start_loc,
                                     top_k=50, top_p=0.9)
    start = start_loc[0] * 4 + start_loc[1]
    assert torch.equal(codes0.view(3, 16, 4)[:, :start], partial.view(3, 16, 4)[:, :start])
    assert not torch.equal(codes0, partial)


def test_composed_per_image_weights(tiny3):
    ar, aux, cond, uncond, extras, zeros = tiny3
    X.check_per_image_weights(ar, aux, zeros, cond, uncond, extras[0], [-2.0, 0.0, 1.25], seeds=[11, 12, 13], top_k=50, top_p=0.9)


def test_composed_log_probs(nat, tiny3):
    ar, aux, cond, uncond, extras, zeros = tiny3
    n = X.check_log_probs(nat, ar, aux, zeros, cond, uncond, extras[:1], [-0.5], seeds=[21, 22, 23])
    assert n >= 1                                          # (slot 0 of an image needs its first code alone to agree)


def test_composed_prefix_one_pass(nat, tiny3):
    ar, aux, cond, uncond, extras, _ = tiny3
    partial = G.random_codes((3, 4, 4, 4), 500, 8, DEV)
    ar.prefix_mode = 'one_pass'
    try:
        M.seed_all(5)
        with ar.extra_conds(conds=extras, weights=list(WEIGHTS2)):
            xs = ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=2.5, top_k=50, start_loc=(1, 2))
    finally:
        ar.prefix_mode = 'stepped'
    assert torch.equal(xs.view(3, 16, 4)[:, :6], partial.view(3, 16, 4)[:, :6])
    drawn = torch.ones((3, 16, 4), dtype=torch.bool)
    drawn[:, :6] = False
    # the support check runs the stepped pass: its logits differ from the one-pass prefill's by GEMM tiles, within the top-50 margin of
    # the guided tests of prefix_mode (a code at the very edge of the support could fall outside; none does for these seeds)
    X.check_composed_support(nat, ar, aux, xs, cond, uncond, extras, WEIGHTS2, 2.5, 50, drawn=drawn.view(3, 4, 4, 4))


def test_composed_schedule_and_truncation(tiny3):
    """a guidance schedule constant over the positions, and min_p off values, return the unscheduled composed call's codes"""
    ar, aux, cond, uncond, extras, zeros = tiny3
    kw = dict(cond=cond, uncond=uncond, top_k=50, top_p=0.9)
    M.seed_all(9)
    with ar.extra_conds(conds=extras[:1], weights=[-1.5]):
        want = ar.sample_guided(zeros, aux, guidance_scale=3.0, **kw)
        M.seed_all(9)
        with ar.schedule(guidance_scale=torch.full((4, 4), 3.0)):
            got = ar.sample_guided(zeros, aux, **kw)
        M.seed_all(9)
        with ar.schedule(guidance_scale=torch.full((4, 4), 3.0)):
            unc = ar.sample_guided(zeros, aux, cached=False, **kw)
        M.seed_all(9)
        tr = ar.sample_guided(zeros, aux, guidance_scale=3.0, min_p=0.05, **kw)
        M.seed_all(9)
        tru = ar.sample_guided(zeros, aux, guidance_scale=3.0, min_p=0.05, cached=False, **kw)
    assert torch.equal(got, want) and torch.equal(unc, want)
    assert torch.equal(tr, tru)


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_composed_refusals(nat, tiny3):
    ar, aux, cond, uncond, extras, zeros = tiny3
    kw = dict(cond=cond, uncond=uncond, guidance_scale=2.0, top_k=50)
    fresh, aux2 = M.model(C.RQT_TINY, 41, DEV)
    M.seed_all(1)
    want = fresh.sample(zeros, aux2, cond=cond, top_k=50)

    def usable():
        M.seed_all(1)
        assert torch.equal(ar.sample(zeros, aux, cond=cond, top_k=50), want)
    vc = 10
    five = [(cond + 1 + k) % vc for k in range(5)]
    with pytest.raises(ValueError, match='extra conditions'):
        with ar.extra_conds(conds=five, weights=[0.5] * 5):
            ar.sample_guided(zeros, aux, **kw)
    usable()
    with pytest.raises(ValueError, match='finite'):
        with ar.extra_conds(conds=extras[:1], weights=[float('nan')]):
            ar.sample_guided(zeros, aux, **kw)
    usable()
    with pytest.raises(ValueError, match='finite'):
        with ar.extra_conds(conds=extras[:1], weights=[torch.tensor([1.0, float('inf'), 0.0])]):
            ar.sample_guided(zeros, aux, **kw)
    with pytest.raises(ValueError, match='weights'):
        with ar.extra_conds(conds=extras, weights=[0.5]):
            ar.sample_guided(zeros, aux, **kw)
    usable()
    with pytest.raises(ValueError, match='shape'):
        with ar.extra_conds(conds=[extras[0][:2]], weights=[0.5]):
            ar.sample_guided(zeros, aux, **kw)
    usable()
    with pytest.raises(NotImplementedError, match='sample_guided'):
        with ar.extra_conds(conds=extras[:1], weights=[0.5]):
            ar.sample(zeros, aux, cond=cond, top_k=50)
    usable()
    with pytest.raises(NotImplementedError, match='shared_cond'):
        with ar.shared_cond(1), ar.extra_conds(conds=extras[:1], weights=[0.5]):
            ar.sample_guided(zeros, aux, **kw)
    usable()
    with pytest.raises(ValueError, match='negative'):
        with ar.extra_conds(conds=extras[:1], weights=[0.5]):
            ar.sample_guided(zeros, aux, negative=extras[1], **kw)
    usable()
    ar.sampler = 'torch'
    try:
        with pytest.raises(NotImplementedError, match='torch'):
            ar.sample_guided(zeros, aux, negative=extras[1], **kw)
    finally:
        ar.sampler = 'philox'
    usable()
    # at the ABI: K = 5 is refused when the call arms; a NaN weight, an unguided call and a shared-prompt arming when the armed call is made,
    # before anything is enqueued -- and each consumes the arming: the guided call that follows is a plain guided call
    import ctypes
    from rqvae._native import _int_array, _ptr_array, ptr
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    L, h = eng._L, eng._h
    D, B = 4, 3
    cb, tk, tp = _ptr_array(cbs[:D]), _int_array([50] * D), (ctypes.c_float * D)(*[1.0] * D)
    out = torch.empty_like(zeros)
    ex = (ctypes.c_void_p * 5)(*[ptr(e).value for e in five])
    w_ok, w_nan = (ctypes.c_float * (5 * B))(*[0.5] * (5 * B)), (ctypes.c_float * B)(0.5, float('nan'), 0.5)

    def guided_call(seed=2):
        return L.rqamd_rqt_sample_guided(h, ptr(zeros), None, None, ptr(cond), ptr(uncond), B, cb, 0, 0, 1.0, 2.0, tk, tp, seed, 0, 0, ptr(out), None)
    torch.cuda.synchronize()
    assert guided_call() == 0
    torch.cuda.synchronize()
    ref = out.clone()
    assert L.rqamd_rqt_sample_compose(h, 5, ex, w_ok) == -1 and b'extra conditions' in L.rqamd_last_error()
    assert guided_call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert L.rqamd_rqt_sample_compose(h, 1, ex, w_nan) == 0
    assert guided_call() == -1 and b'finite' in L.rqamd_last_error()
    assert guided_call() == 0                              # (the refused call consumed the arming)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert L.rqamd_rqt_sample_compose(h, 1, ex, w_ok) == 0
    assert L.rqamd_rqt_sample(h, ptr(zeros), ptr(cond), B, cb, 0, 0, 1.0, tk, tp, 2, 0, 0, ptr(out), None) == -1 and b'unguided' in L.rqamd_last_error()
    assert L.rqamd_rqt_sample_compose(h, 1, ex, w_ok) == 0 and L.rqamd_rqt_sample_shared(h, 1) == 0
    assert guided_call() == -2 and b'rqamd_rqt_sample_shared' in L.rqamd_last_error()
    assert L.rqamd_rqt_sample_compose(h, 1, ex, w_ok) == 0 and L.rqamd_rqt_sample_compose(h, 0, None, None) == 0      # disarmed
    assert guided_call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    usable()
