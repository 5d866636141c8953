"""Per-image sampling parameters and seeds on the MI355X (`pytest -m gpu`): rqamd_sample_logits_rows, rqamd_rqt_sample_rows, the tensor
arguments of RQTransformer.sample / sample_guided and RQTransformer.seeds().  Row r of a per-row call is held, bit for bit, against the
entry point that takes one value per call, made with r's values; only the comparison with the oracle has a tolerance.  Captured graphs
are on unless a test says otherwise."""
import os
import sys

import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402
import per_image_sampling_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
B = 6


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


@pytest.fixture(scope='module')
def tiny(nat):
    """RQT_TINY (4x4x4, V 500) with seeded weights, 6 images"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond), torch.zeros((B, 4, 4, 4), dtype=torch.long, device=DEV)


def _codes(seed=3):
    return G.random_codes((B, 4, 4, 4), 500, seed, DEV)


# ---------------------------------------------------------------------------------------------- 1. kernel: rows against the scalar entry point
@pytest.mark.parametrize('want_probs', [False, True])
@pytest.mark.parametrize('V', P.VOCABS)
def test_rows_equal_scalar_calls(nat, V, want_probs):
    P.check_rows_against_scalar(nat, V, DEV, want_probs)


@pytest.mark.parametrize('V', P.VOCABS)
def test_row_seeds(nat, V):
    P.check_row_seeds(nat, V, DEV)


# ---------------------------------------------------------------------------------------------- 2. kernel against the oracle
def test_rows_against_oracle(nat):
    P.check_rows_against_oracle(nat, DEV)


# ---------------------------------------------------------------------------------------------- 3. heterogeneous call == homogeneous calls
@pytest.mark.parametrize('amp', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('form', ['plain', 'per_depth', 'keep_mask', 'start_loc'])
def test_hetero_equals_homogeneous(tiny, form, amp):
    ar, aux, cond, _, zeros = tiny
    extra = dict(amp=amp)
    partial = zeros
    if form == 'keep_mask':
        extra['keep_mask'] = torch.from_numpy(M.replay_mask(B, 4, 4, 4, 9)).to(DEV)
        partial = _codes(4)
    if form == 'start_loc':
        extra['start_loc'] = (1, 2)
        partial = _codes(5)
    got, outs = P.check_hetero(ar, aux, partial, cond, seed=5, per_depth=form == 'per_depth', **extra)
    assert not torch.equal(outs[0], outs[1])               # the groups do draw different codes
    if form == 'start_loc':
        assert torch.equal(got.view(B, 16, 4)[:, :6], partial.view(B, 16, 4)[:, :6])


@pytest.mark.parametrize('amp', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('form', ['plain', 'keep_mask', 'start_loc'])
def test_hetero_guided_equals_homogeneous(tiny, form, amp):
    ar, aux, cond, uncond, zeros = tiny
    extra = dict(amp=amp)
    partial = zeros
    if form == 'keep_mask':
        extra['keep_mask'] = torch.from_numpy(M.replay_mask(B, 4, 4, 4, 9)).to(DEV)
        partial = _codes(4)
    if form == 'start_loc':
        extra['start_loc'] = (1, 2)
        partial = _codes(5)
    P.check_hetero(ar, aux, partial, cond, seed=7, uncond=uncond, **extra)


# ---------------------------------------------------------------------------------------------- 4. seeds
def test_seeds(tiny):
    ar, aux, cond, _, zeros = tiny
    codes = _codes(6)
    perm = torch.tensor([4, 2, 5, 0, 3, 1], device=DEV)
    P.check_position_independent_logits(ar, aux, codes, cond, perm)
    seeds = [11, 2 ** 40 + 3, 5, 11, 0, 77]
    keep = G.few_mask(B).to(DEV)
    none = torch.zeros((B, 4, 4, 4), dtype=torch.bool, device=DEV)
    for km in (none, keep):
        out = P.check_seed_permutation(ar, aux, codes, cond, seeds, perm, keep_mask=km)
        for b in (0, 4):
            P.check_seed_single_image(ar, aux, codes, cond, seeds, out, b, km)
    P.check_seed_streams(ar, aux, codes, cond, lambda: torch.cuda.get_rng_state(DEV))


def test_seeds_guided_permutation(tiny):
    ar, aux, cond, uncond, zeros = tiny
    kw = P.group_tensors(B, 500, DEV)
    kw['guidance_scale'] = torch.tensor([P.SCALES[i] for i in P.group_of(B)], device=DEV)
    seeds = [3, 1, 4, 1, 5, 9]
    perm = torch.tensor([5, 3, 1, 0, 2, 4], device=DEV)
    with ar.seeds(seeds):
        a = ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, **kw)
    with ar.seeds([seeds[i] for i in perm.tolist()]):
        b = ar.sample_guided(zeros, aux, cond=cond[perm].contiguous(), uncond=uncond[perm].contiguous(), **{k: v[perm].contiguous() for k, v in kw.items()})
    assert torch.equal(b, a[perm])


# ---------------------------------------------------------------------------------------------- 5. graphs
def test_graphs_hold_no_values(tiny):
    ar, aux, cond, _, zeros = tiny
    eng = ar._eng(False)
    Pk = P.group_tensors(B, 500, DEV)
    Qk = dict(temperature=Pk['temperature'].flip(0).contiguous() * 0.9, top_k=Pk['top_k'].flip(0).contiguous(), top_p=Pk['top_p'].flip(0).contiguous())
    scalar = dict(temperature=0.9, top_k=40, top_p=0.95)

    def run(kw, graph):
        ar.use_graph = graph
        try:
            M.seed_all(13)
            return ar.sample(zeros, aux, cond=cond, **kw)
        finally:
            ar.use_graph = True
    a1 = run(Pk, True)
    n_after_a = eng.graph_captures()
    b = run(Qk, True)
    assert eng.graph_captures() == n_after_a, 'a per-image call with other values captured graphs again'
    s = run(scalar, True)
    n_after_s = eng.graph_captures()
    a2 = run(Pk, True)
    s2 = run(scalar, True)
    assert eng.graph_captures() == n_after_s, 'scalar and per-image calls invalidate each other\'s graphs'
    assert torch.equal(a1, run(Pk, False)) and torch.equal(b, run(Qk, False)) and torch.equal(s, run(scalar, False))
    assert torch.equal(a1, a2) and torch.equal(s, s2)
    assert not torch.equal(a1, b)
    # seeded calls after unseeded ones (and back): a seeded launch reads another key buffer, so it must not replay an unseeded graph
    seeds = [3, 1, 4, 1, 5, 9]

    def run_seeded(graph):
        with ar.seeds(seeds):
            return run(Pk, graph)
    c1 = run_seeded(True)
    n_after_c = eng.graph_captures()
    a3 = run(Pk, True)
    c2 = run_seeded(True)
    assert eng.graph_captures() == n_after_c, 'seeded and unseeded per-image calls invalidate each other\'s graphs'
    assert torch.equal(c1, run_seeded(False)) and torch.equal(c1, c2) and torch.equal(a1, a3)
    assert not torch.equal(c1, a1)


def test_graphs_seeded_after_unseeded_guided(tiny):
    """the guided family likewise: unseeded per-image graphs are there when the first seeded call comes"""
    ar, aux, cond, uncond, zeros = tiny
    kw = dict(cond=cond, uncond=uncond, guidance_scale=torch.tensor([P.SCALES[i] for i in P.group_of(B)], device=DEV), **P.group_tensors(B, 500, DEV))
    M.seed_all(3)
    ar.sample_guided(zeros, aux, **kw)
    with ar.seeds(list(range(B))):
        a = ar.sample_guided(zeros, aux, **kw)
        ar.use_graph = False
        try:
            b = ar.sample_guided(zeros, aux, **kw)
        finally:
            ar.use_graph = True
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 6. host loops
def test_host_loops(nat, tiny):
    ar, aux, cond, uncond, _ = tiny
    keep = P.three_code_mask(B).to(DEV)
    partial = torch.where(keep, _codes(5), torch.full((), M.OUT_OF_RANGE, dtype=torch.long, device=DEV))
    kw = dict(cond=cond, keep_mask=keep, **P.group_tensors(B, 500, DEV))
    M.seed_all(7)
    a = ar.sample(partial, aux, **kw)
    M.seed_all(7)
    b = ar.sample(partial, aux, cached=False, **kw)
    assert torch.equal(a, b)                               # the cache changes nothing, per image as per call
    assert torch.equal(a[keep], partial[keep])
    with ar.seeds(list(range(B))):
        c = ar.sample(partial, aux, **kw)
        d = ar.sample(partial, aux, cached=False, **kw)
    assert torch.equal(c, d)
    gkw = dict(kw, uncond=uncond, guidance_scale=torch.tensor([P.SCALES[i] for i in P.group_of(B)], device=DEV))
    M.seed_all(7)
    e = ar.sample_guided(partial, aux, **gkw)
    M.seed_all(7)
    f = ar.sample_guided(partial, aux, cached=False, **gkw)
    assert torch.equal(e, f)
    ar.sampler = 'torch'
    try:
        M.seed_all(7)
        t = ar.sample(partial, aux, **kw)
        with pytest.raises(ValueError, match='seeds'):
            with ar.seeds(list(range(B))):
                ar.sample(partial, aux, **kw)
    finally:
        ar.sampler = 'philox'
    assert torch.equal(t[keep], partial[keep])
    P.check_torch_support(nat, ar, aux, t, cond, keep)


# ---------------------------------------------------------------------------------------------- 7. errors
def test_errors(nat, tiny):
    ar, aux, cond, uncond, _ = tiny
    partial = _codes()
    ones = torch.ones((B, 4, 4, 4), dtype=torch.bool, device=DEV)
    for name, kw in P.value_error_cases(B, 4, 500, DEV):
        with pytest.raises(ValueError):
            ar.sample(partial, aux, cond=cond, keep_mask=ones, **kw)
        pytest.raises(ValueError, ar.sample_guided, partial, aux, cond=cond, uncond=uncond, keep_mask=ones, **kw)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite'):
            ar.sample_guided(partial, aux, cond=cond, uncond=uncond, keep_mask=ones, guidance_scale=torch.tensor([1.0] * (B - 1) + [bad]))
    for bad in ([-1] + [0] * (B - 1), torch.tensor([-5] * B), torch.ones(B), [1] * (B + 1)):
        with pytest.raises(ValueError):
            with ar.seeds(bad):
                ar.sample(partial, aux, cond=cond, keep_mask=ones)
    assert torch.equal(ar.sample(partial, aux, cond=cond, keep_mask=ones, temperature=torch.ones(B)), partial)
    T, k, p = [1.0] * B, [10] * (B * 4), [0.9] * (B * 4)
    assert P.c_sample_rows(nat, ar, aux, partial, cond, T, k, p)[0] == 0
    for null in ('T', 'k', 'p'):
        rc, msg = P.c_sample_rows(nat, ar, aux, partial, cond, T, k, p, null=(null,))
        assert rc == -1 and b'null' in msg, null
    rc, msg = P.c_sample_rows(nat, ar, aux, partial, cond, T[:-1] + [0.0], k, p)
    assert rc == -1 and b'temperature' in msg
    rc, msg = P.c_sample_rows(nat, ar, aux, partial, cond, T, k, p, scale=[1.0] * (B - 1) + [float('inf')])
    assert rc == -1 and b'finite' in msg
