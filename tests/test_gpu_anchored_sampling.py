"""Anchored sampling on the MI355X (`pytest -m gpu`): RQTransformer.anchor over rqamd_rqt_sample_anchor, and rqamd_anchor_logits.  At every
head step of an anchored call three launches (residual of the image given the codes so far, the quantiser's distance kernel, fold) write
logits - w * dist to a scratch the sampler reads.  Apart from the fold against fp64 every comparison is exact.  Captured graphs are on
unless a test says otherwise."""
import os
import sys

import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchored_sampling_cases as A  # noqa: E402
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


_SETUPS = {}


def _setup(B):
    """the tiny model (4x4x4, V 500, dim 64) with the quantiser of the soft-loss fixture, B images: one per batch size, shared"""
    if B not in _SETUPS:
        ar, aux, cond, z = A.setup(DEV, B)
        _SETUPS[B] = (ar, aux, cond, z, torch.zeros((B, 4, 4, 4), dtype=torch.long, device=DEV))
    return _SETUPS[B]


@pytest.fixture(scope='module')
def tiny3(nat):
    return _setup(3)


def _weight(kind, B):
    return {'scalar': 2.0, 'per_depth': A.PER_DEPTH, 'table': A.image_table(B)}[kind]


# ---------------------------------------------------------------------------------------------- 1. anchor_logits alone
@pytest.mark.parametrize('shape', [(1, 499, 64), (3, 500, 64), (257, 16384, 256)])
@pytest.mark.parametrize('d', [0, 3])
def test_anchor_logits(nat, shape, d):
    A.check_anchor_logits(nat, *shape, d, DEV, seed=shape[1] + d)


# ---------------------------------------------------------------------------------------------- 2. zero weight is the plain call
@pytest.mark.parametrize('use_graph', [True, False])
def test_anchor_zero_weight_is_the_plain_call(tiny3, use_graph):
    ar, aux, cond, z, zeros = tiny3
    uncond = G.uncond_for(C.RQT_TINY, cond)
    keep = torch.from_numpy(M.replay_mask(3, 4, 4, 4, 21)).to(DEV)
    partial = G.random_codes((3, 4, 4, 4), 500, 6, DEV)

    def per_image():
        with ar.seeds([11, 12, 13]):
            return ar.sample(zeros, aux, cond=cond, temperature=torch.tensor([0.8, 1.0, 1.3]), top_k=torch.tensor([50, 500, 20]),
                             top_p=torch.tensor([0.9, 1.0, 0.95]))

    def logp():
        with ar.return_log_probs():
            return ar.sample(zeros, aux, cond=cond, top_k=50, top_p=0.9)

    def logp_guided():
        with ar.return_log_probs():
            return ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=3.0, top_k=50)
    ar.use_graph = use_graph
    try:
        for name in sorted(M.SAMPLERS):
            A.check_zero_weight(ar, z, lambda: ar.sample(zeros, aux, cond=cond, **M.SAMPLERS[name]), seed=5)
        A.check_zero_weight(ar, z, lambda: ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=3.0, top_k=50, top_p=0.9), seed=6,
                            weight=torch.zeros((3, 4, 4, 4)))
        A.check_zero_weight(ar, z, lambda: ar.sample(partial, aux, cond=cond, keep_mask=keep, top_k=50), seed=7, weight=[0.0] * 4)
        A.check_zero_weight(ar, z, per_image, seed=8, weight=torch.zeros((4, 4)))
        A.check_zero_weight(ar, z, logp, seed=9)
        A.check_zero_weight(ar, z, logp_guided, seed=10, weight=torch.zeros((3,)))
    finally:
        ar.use_graph = True


# ---------------------------------------------------------------------------------------------- 3. engine == host loop
def _host_loop(B, kind, run, seed, plain=None):
    """cached=True with graphs on and off == cached=False, inside anchor(z, weight)"""
    ar, aux, cond, z, zeros = _setup(B)
    w = _weight(kind, B)
    a = A.check_host_loop(ar, z, w, lambda cached: run(ar, aux, cond, zeros, cached), seed, differs_from=plain)
    ar.use_graph = False
    try:
        M.seed_all(seed)
        with ar.anchor(z, w):
            b = run(ar, aux, cond, zeros, True)
    finally:
        ar.use_graph = True
    assert torch.equal(a, b), 'captured graphs and eager launches differ'
    return a


@pytest.mark.parametrize('B,kind', [(3, 'scalar'), (3, 'per_depth'), (3, 'table'), (5, 'table')])
def test_anchor_sample_equals_host_loop(nat, B, kind):
    ar, aux, cond, z, zeros = _setup(B)
    M.seed_all(7)
    plain = ar.sample(zeros, aux, cond=cond)
    _host_loop(B, kind, lambda ar, aux, cond, zeros, cached: ar.sample(zeros, aux, cond=cond, cached=cached), 7, plain=plain)


def test_anchor_topk_topp_equals_host_loop(nat):
    _host_loop(5, 'per_depth', lambda ar, aux, cond, zeros, cached: ar.sample(zeros, aux, cond=cond, top_k=50, top_p=0.9, cached=cached), 8)


@pytest.mark.parametrize('scale,B,kind', [(0.0, 3, 'table'), (1.0, 5, 'scalar'), (3.0, 3, 'per_depth')])
def test_anchor_guided_equals_host_loop(nat, scale, B, kind):
    def run(ar, aux, cond, zeros, cached):
        return ar.sample_guided(zeros, aux, cond=cond, uncond=G.uncond_for(C.RQT_TINY, cond), guidance_scale=scale, top_k=50, top_p=0.9, cached=cached)
    _host_loop(B, kind, run, 9)


def test_anchor_keep_mask_equals_host_loop(nat):
    """the replay mask: kept depth-0 codes that are not the image's own, so the residual must follow the given code; fillers out of range"""
    keep = torch.from_numpy(M.replay_mask(3, 4, 4, 4, 21)).to(DEV)
    given = G.random_codes((3, 4, 4, 4), 500, 6, DEV)
    partial = torch.where(keep, given, torch.full_like(given, M.OUT_OF_RANGE))

    def run(ar, aux, cond, zeros, cached):
        return ar.sample(partial, aux, cond=cond, keep_mask=keep, top_k=50, cached=cached)
    got = _host_loop(3, 'table', run, 10)
    assert torch.equal(got[keep], given[keep])


@pytest.mark.parametrize('prefix_mode', ['stepped', 'one_pass'])
def test_anchor_start_loc_equals_host_loop(nat, prefix_mode):
    given = G.random_codes((5, 4, 4, 4), 500, 8, DEV)

    def run(ar, aux, cond, zeros, cached):
        # (the host loop steps every position; 'one_pass' fills the KV rows of the 9 given positions through other GEMM tiles, which
        #  moves no draw of this seed)
        ar.prefix_mode = prefix_mode
        try:
            return ar.sample(given, aux, cond=cond, start_loc=(2, 1), top_k=50, cached=cached)
        finally:
            ar.prefix_mode = 'stepped'
    got = _host_loop(5, 'scalar', run, 11)
    assert torch.equal(got.view(5, 16, 4)[:, :9], given.view(5, 16, 4)[:, :9])


def test_anchor_truncation_and_schedule_equal_host_loop(nat):
    _host_loop(3, 'scalar', lambda ar, aux, cond, zeros, cached: ar.sample(zeros, aux, cond=cond, top_k=50, min_p=0.05, cached=cached), 12)

    def scheduled(ar, aux, cond, zeros, cached):
        with ar.schedule(temperature=ar.position_ramp(1.3, 0.7)):
            return ar.sample(zeros, aux, cond=cond, top_k=50, cached=cached)
    _host_loop(3, 'per_depth', scheduled, 13)


def test_anchor_amp_equals_host_loop(nat):
    _host_loop(3, 'table', lambda ar, aux, cond, zeros, cached: ar.sample(zeros, aux, cond=cond, top_k=50, top_p=0.9, amp=True, cached=cached), 14)


def test_anchor_log_probs(nat, tiny3):
    ar, aux, cond, z, zeros = tiny3
    tab = A.image_table(3)
    n = A.check_log_probs(nat, ar, aux, zeros, cond, z, tab, tab, seeds=[21, 22, 23])
    assert n == zeros.numel()


# ---------------------------------------------------------------------------------------------- 4. a strong anchor returns the image's codes
def test_strong_anchor_returns_the_image_codes(nat, tiny3):
    ar, aux, cond, _, _ = tiny3
    k, z = A.strong_anchor_inputs(aux, 3, 17, DEV)
    A.check_strong_anchor(nat, ar, aux, cond, k, z)


# ---------------------------------------------------------------------------------------------- 5. graphs
def test_anchor_graph_captures(nat):
    """an anchored call, an anchored call with other z and other weights, a plain call, an anchored call again, on a handle of their own:
    only the first anchored call and the first plain call capture; equal calls return equal codes, other weights other codes"""
    ar, aux, cond, z = A.setup(DEV, 3)
    zeros = torch.zeros((3, 4, 4, 4), dtype=torch.long, device=DEV)
    z2 = z.flip(0).contiguous()

    def anchored(zz, w):
        M.seed_all(2)
        with ar.anchor(zz, w):
            return ar.sample(zeros, aux, cond=cond, top_k=50, top_p=0.9)

    def plain():
        M.seed_all(2)
        return ar.sample(zeros, aux, cond=cond, top_k=50, top_p=0.9)
    a1 = anchored(z, 2.0)
    eng = ar._eng(False)
    n1 = eng.graph_captures()
    assert n1 > 0
    a2 = anchored(z2, A.image_table(3))
    assert eng.graph_captures() == n1, 'another z / other weights recaptured graphs'
    p1 = plain()
    n2 = eng.graph_captures()
    assert n2 > n1
    a3 = anchored(z, 2.0)
    p2 = plain()
    assert eng.graph_captures() == n2, 'alternating anchored and plain calls recaptured graphs'
    assert torch.equal(a1, a3) and torch.equal(p1, p2)
    assert not torch.equal(a1, a2) and not torch.equal(a1, p1)
    fresh, aux2, _, _ = A.setup(DEV, 3)
    M.seed_all(2)
    assert torch.equal(fresh.sample(zeros, aux2, cond=cond, top_k=50, top_p=0.9), p1)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_anchor_refusals(nat, tiny3):
    ar, aux, cond, z, zeros = tiny3
    fresh, aux2, _, _ = A.setup(DEV, 3)
    M.seed_all(1)
    want = fresh.sample(zeros, aux2, cond=cond, top_k=50)

    def usable():
        M.seed_all(1)
        assert torch.equal(ar.sample(zeros, aux, cond=cond, top_k=50), want)
    A.check_refusals(ar, aux, cond, z, zeros, usable)
    A.check_tuple_refused(DEV, z)
    A.check_abi_refusals(nat, ar, aux, cond, z, zeros, sync=torch.cuda.synchronize)
    usable()
