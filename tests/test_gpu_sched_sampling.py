"""Sampling schedules over positions and depths on the MI355X (`pytest -m gpu`): rqamd_rqt_sample_schedule through
RQTransformer.schedule() on the tiny fixture models -- the scheduled sampler kernels (rqt_sample_sched.hip) in their plain, LOGP and
TRUNC builds, unguided and guided, over the shared and the per-image tables.  Constant schedules against the per-image and the scalar
call, every table index replayed by the stand-alone per-row sampler, replay through masks, graph == eager == cached=False, graph
accounting, the effect of a schedule, refusals.  Every comparison is exact (tests/sched_sampling_cases.py)."""
import pytest
import torch

import guided_sampling_cases as G
import masked_sampling_cases as M
import sched_sampling_cases as sc
from oracle import configs as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = sc.B


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


@pytest.fixture(scope='module')
def tiny(nat):
    """RQT_TINY (4x4x4, V 500) with seeded weights, 3 images; sample() takes (SEED, OFFSET) in place of the generator's state"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    sc.fix_rng(ar)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond)


# ---------------------------------------------------------------------------------------------- 1. constant == per-image == scalar
@pytest.mark.parametrize('amp', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('form', ['plain', 'masked', 'guided', 'guided_masked', 'seeds', 'trunc', 'guided_trunc'])
def test_constant_schedule(nat, tiny, form, amp):
    ar, aux, cond, uncond = tiny
    keep = torch.from_numpy(M.replay_mask(B, 4, 4, 4, 7)) if 'masked' in form else None
    seeds = [11, 2 ** 40 + 5, 11] if form == 'seeds' else None
    sc.check_constant(ar, aux, cond, keep, uncond if 'guided' in form else None, seeds, 'trunc' in form, amp)


# ---------------------------------------------------------------------------------------------- 2. every index, by replay
@pytest.mark.parametrize('guided', [False, True], ids=['plain', 'guided'])
@pytest.mark.parametrize('trunc', [False, True], ids=['filters', 'trunc'])
@pytest.mark.parametrize('per_image', [False, True], ids=['shared', 'per_image'])
def test_replay_every_index(nat, tiny, per_image, trunc, guided):
    ar, aux, cond, uncond = tiny
    sc.check_replay_every_index(nat, ar, aux, cond, per_image, trunc, None, uncond if guided else None)


def test_replay_every_index_seeded_text(nat):
    """the text-conditioned fixture (2 images), guided, per-image seeds next to a shared schedule: the per-image table, key seeds[b]"""
    ar, aux = M.model(C.RQT_TINY_TXT, 43, DEV)
    cond = M.cond_for(C.RQT_TINY_TXT, 2, DEV)
    uncond = G.uncond_for(C.RQT_TINY_TXT, cond)
    assert tuple(ar.block_size) == (sc.H, sc.W, sc.D) and max(ar.vocab_size) == sc.V
    sched = sc.distinct_schedule(False, True, True, b=2)
    seeds = [2 ** 63 + 11, 7]
    with ar.schedule(**sched), ar.seeds(seeds), ar.return_log_probs():
        X, lp = sc.call(ar, aux, cond, None, uncond)
    sc.replay(nat, ar, aux, cond, sched, X, lp.draw, None, uncond, seeds=seeds)


# ---------------------------------------------------------------------------------------------- 3. replay through masks
@pytest.mark.parametrize('guided', [False, True], ids=['plain', 'guided'])
def test_replay_through_masks(nat, tiny, guided):
    ar, aux, cond, uncond = tiny
    u = uncond if guided else None
    sched = sc.distinct_schedule(True, True, False, depth_T=False)
    if guided:
        sched['guidance_scale'] = (0.5 + 0.1 * torch.arange(B * 16, dtype=torch.float32)).view(B, 4, 4, 1).expand(B, 4, 4, 4).clone()
    with ar.schedule(**sched):
        X = sc.call(ar, aux, cond, None, u)
    sc.check_position_by_per_image_call(ar, aux, cond, X, sched, (0, 5, 15), u)
    if not guided:
        with ar.schedule(**sched):
            assert torch.equal(M.check_replay(ar, aux, cond, M.replay_mask(B, 4, 4, 4, 7), 5), X)


# ---------------------------------------------------------------------------------------------- 4. graph == eager == cached=False
@pytest.mark.parametrize('amp', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('per_image', [False, True], ids=['shared', 'per_image'])
def test_paths(nat, tiny, per_image, amp):
    ar, aux, cond, uncond = tiny
    sched = sc.distinct_schedule(per_image, True, False)
    given = G.random_codes((B, 4, 4, 4), 500, 3, DEV)
    prefix = lambda t: t.view(B, 16, 4)[:, :9]
    with ar.schedule(**sched):
        a = sc.call(ar, aux, cond, amp=amp)
        s1 = ar.sample(given, aux, cond=cond, start_loc=(2, 1), amp=amp)
        ar.use_graph = False
        try:
            assert torch.equal(sc.call(ar, aux, cond, amp=amp), a), 'graph and eager calls differ'
            assert torch.equal(ar.sample(given, aux, cond=cond, start_loc=(2, 1), amp=amp), s1), 'start_loc: graph and eager calls differ'
        finally:
            ar.use_graph = True
        if not amp:
            assert torch.equal(sc.call(ar, aux, cond, cached=False), a), 'cached=False differs from the cached call'
            assert torch.equal(ar.sample(given, aux, cond=cond, start_loc=(2, 1), cached=False), s1), 'start_loc: cached=False differs'
        assert torch.equal(prefix(s1), prefix(given)) and not torch.equal(s1, given)
        saved, ar.prefix_mode = ar.prefix_mode, 'one_pass'
        try:
            s2 = ar.sample(given, aux, cond=cond, start_loc=(2, 1), amp=amp)
            ar.use_graph = False
            s3 = ar.sample(given, aux, cond=cond, start_loc=(2, 1), amp=amp)
        finally:
            ar.prefix_mode, ar.use_graph = saved, True
        assert torch.equal(s2, s3), 'one_pass: graph and eager calls differ'
        assert torch.equal(prefix(s2), prefix(given)), 'one_pass: the given prefix changed'


def test_paths_guided_uncached(nat, tiny):
    ar, aux, cond, uncond = tiny
    sched = sc.distinct_schedule(True, False, True)
    with ar.schedule(**sched):
        a = sc.call(ar, aux, cond, None, uncond)
        assert torch.equal(sc.call(ar, aux, cond, None, uncond, cached=False), a), 'guided: cached=False differs from the cached call'


# ---------------------------------------------------------------------------------------------- 5. graph accounting
def test_graph_accounting(nat):
    """another schedule replays the same graphs; scalar, per-image and scheduled calls never recapture each other's; the shared and the
    per-image table have graph sets of their own"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)                # a model of its own: no graph of an earlier test
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    sc.fix_rng(ar)
    eng = ar._eng(False)
    kw = dict(temperature=sc.CONST_T, top_k=sc.CONST_K, top_p=sc.CONST_P)
    rows = dict(kw, temperature=torch.tensor([0.9, 0.8, 1.0], device=DEV))
    s_a, s_b = sc.distinct_schedule(False, False, False), dict(temperature=ar.position_ramp(1.2, 0.6), top_k=torch.full((4, 4), 40))
    p_a, p_b = sc.distinct_schedule(True, False, False), dict(top_p=torch.full((B, 4, 4, 4), 0.8))

    def run(sched=None, **k):
        if sched is None:
            return sc.call(ar, aux, cond, **k)
        with ar.schedule(**sched):
            return sc.call(ar, aux, cond, **k)
    scalar = run(**kw)
    n0 = eng.graph_captures()
    per_image = run(**rows)
    n1 = eng.graph_captures()
    first = run(s_a)
    n2 = eng.graph_captures()
    assert 0 < n0 < n1 < n2
    other = run(s_b)
    assert eng.graph_captures() == n2, 'a second scheduled call with other values captured graphs'
    assert not torch.equal(first, other)
    for _ in range(2):
        assert torch.equal(run(**kw), scalar) and torch.equal(run(**rows), per_image) and torch.equal(run(s_a), first)
    assert eng.graph_captures() == n2, 'alternating scheduled, scalar and per-image calls recaptured'
    pi_first = run(p_a)
    n3 = eng.graph_captures()
    assert n3 > n2, 'the per-image table replayed graphs of the shared one'
    run(p_b)
    assert torch.equal(run(s_a), first) and torch.equal(run(p_a), pi_first) and torch.equal(run(**kw), scalar) and torch.equal(run(**rows), per_image)
    # a shared schedule next to a per-image argument uses the per-image table: the same graphs
    run(s_b, top_p=torch.tensor([0.9, 0.8, 1.0], device=DEV))
    assert eng.graph_captures() == n3, 'calls after the first of each kind recaptured'
    keep = torch.from_numpy(M.replay_mask(B, 4, 4, 4, 7))
    with ar.schedule(**s_a):
        sc.call(ar, aux, cond, keep)
    n4 = eng.graph_captures()
    with ar.schedule(**s_b):
        sc.call(ar, aux, cond, keep)
    assert n4 > n3 and eng.graph_captures() == n4 and torch.equal(run(s_a), first) and eng.graph_captures() == n4


# ---------------------------------------------------------------------------------------------- 6. effect
def test_effect(nat, tiny):
    ar, aux, cond, uncond = tiny
    sc.check_greedy_from(ar, aux, cond, 8)
    sc.check_guidance_halves(nat, ar, aux, cond, uncond, 8)


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(nat, tiny):
    ar, aux, cond, uncond = tiny
    sc.check_refusals(ar, aux, cond, uncond)
    sc.check_c_refusals(nat, ar, aux, cond, G.few_mask(B))


# ---------------------------------------------------------------------------------------------- 8. position_ramp
def test_position_ramp(nat, tiny):
    ar = tiny[0]
    sc.check_position_ramp(ar)
    with ar.schedule(guidance_scale=ar.position_ramp(1.0, 4.0, 'cosine'), temperature=ar.position_ramp(1.0, 0.7)):
        out = sc.call(ar, aux=tiny[1], cond=tiny[2], uncond=tiny[3])
    assert out.shape == (B, 4, 4, 4)
