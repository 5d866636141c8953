"""CPU-only checks of per-image sampling parameters and seeds (rqamd_sample_logits_rows, rqamd_rqt_sample_rows, the tensor arguments of
RQTransformer.sample / sample_guided, RQTransformer.seeds) through the host emulator (tests/emu): the same .hip sources executed by
fibers.  Apart from the comparison with the oracle every comparison is exact.  The authoritative runs, with captured graphs, the fp16
engine and full passes, are the `-m gpu` ones (tests/test_gpu_per_image_sampling.py).  A 16-position pass of the tiny model takes the
emulator most of a minute, so the engine calls here carry a keep_mask that leaves three positions to run."""
import os
import sys

import pytest
import torch

from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402
import per_image_sampling_cases as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
DEV = torch.device('cpu')
B = 6


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
    """RQT_TINY (4x4x4, V 500) with seeded weights, 6 images, cond and an uncond that differs from it in every row"""
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    ar.use_graph = False                                  # (the emulator has no stream capture)
    cond = M.cond_for(C.RQT_TINY, B, DEV)
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond)


def _codes(seed=3, n=B):
    return G.random_codes((n, 4, 4, 4), 500, seed, DEV)


# ---------------------------------------------------------------------------------------------- 1. kernel: rows against the scalar entry point
@pytest.mark.parametrize('want_probs', [False, True])
@pytest.mark.parametrize('V', P.VOCABS)
def test_emu_rows_equal_scalar_calls(nat, V, want_probs):
    P.check_rows_against_scalar(nat, V, DEV, want_probs)


@pytest.mark.parametrize('V', P.VOCABS)
def test_emu_row_seeds(nat, V):
    P.check_row_seeds(nat, V, DEV)


# ---------------------------------------------------------------------------------------------- 2. kernel against the oracle
def test_emu_rows_against_oracle(nat):
    P.check_rows_against_oracle(nat, DEV)


# ---------------------------------------------------------------------------------------------- 3. heterogeneous call == homogeneous calls
def test_emu_hetero_plain(nat, tiny):
    ar, aux, cond, _ = tiny
    got, outs = P.check_hetero(ar, aux, _codes(), cond, seed=5, keep_mask=G.few_mask(B))
    assert not torch.equal(outs[0], outs[1])               # the groups do draw different codes


def test_emu_hetero_guided(nat, tiny):
    ar, aux, cond, uncond = tiny
    P.check_hetero(ar, aux, _codes(4), cond, seed=7, uncond=uncond, keep_mask=G.few_mask(B), per_depth=True)


# ---------------------------------------------------------------------------------------------- 4. seeds
def test_emu_seeds(nat, tiny):
    """(three images, one of each group: the teacher-forced passes of the first check are full passes of the emulator)"""
    ar, aux, cond, _ = tiny
    n = 3
    codes, keep, cond = _codes(6, n), G.few_mask(n), cond[:n].contiguous()
    perm = torch.tensor([2, 0, 1])
    P.check_position_independent_logits(ar, aux, codes, cond, perm)
    seeds = [11, 2 ** 40 + 3, 11]
    out = P.check_seed_permutation(ar, aux, codes, cond, seeds, perm, keep_mask=keep)
    P.check_seed_single_image(ar, aux, codes, cond, seeds, out, 1, keep, direct=True)
    P.check_seed_streams(ar, aux, codes, cond, torch.get_rng_state, keep_mask=keep[1])


# ---------------------------------------------------------------------------------------------- 6. host loops
def test_emu_host_loops(nat, tiny):
    """(three images, one of each group, and three codes to draw: the uncached loop runs one full pass of the emulator for each; the
    seeded uncached loop runs on the GPU only)"""
    ar, aux, cond, _ = tiny
    n = 3
    keep, cond = P.three_code_mask(n), cond[:n].contiguous()
    partial = torch.where(keep, _codes(5, n), torch.full((), M.OUT_OF_RANGE, dtype=torch.long))
    kw = dict(cond=cond, keep_mask=keep, **P.group_tensors(n, 500, DEV))
    M.seed_all(7)
    a = ar.sample(partial, aux, **kw)
    M.seed_all(7)
    b = ar.sample(partial, aux, cached=False, **kw)
    assert torch.equal(a, b)                               # the cache changes nothing, per image as per call
    assert torch.equal(a[keep], partial[keep])
    ar.sampler = 'torch'
    try:
        M.seed_all(7)
        t = ar.sample(partial, aux, **kw)
        with pytest.raises(ValueError, match='seeds'):
            with ar.seeds(list(range(n))):
                ar.sample(partial, aux, **kw)
    finally:
        ar.sampler = 'philox'
    assert torch.equal(t[keep], partial[keep])
    P.check_torch_support(nat, ar, aux, t, cond, keep)


# ---------------------------------------------------------------------------------------------- 7. errors
def test_emu_errors(nat, tiny):
    ar, aux, cond, uncond = tiny
    partial = _codes()
    ones = torch.ones((B, 4, 4, 4), dtype=torch.bool)
    for name, kw in P.value_error_cases(B, 4, 500, DEV):
        with pytest.raises(ValueError):
            ar.sample(partial, aux, cond=cond, keep_mask=ones, **kw)
        pytest.raises(ValueError, ar.sample_guided, partial, aux, cond=cond, uncond=uncond, keep_mask=ones, **kw)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite'):
            ar.sample_guided(partial, aux, cond=cond, uncond=uncond, keep_mask=ones, guidance_scale=torch.tensor([1.0] * (B - 1) + [bad]))
    with pytest.raises(ValueError, match='shape'):
        ar.sample_guided(partial, aux, cond=cond, uncond=uncond, keep_mask=ones, guidance_scale=torch.ones(B + 1))
    for bad in ([-1] + [0] * (B - 1), torch.tensor([-5] * B), torch.ones(B), [1] * (B + 1)):
        with pytest.raises(ValueError):
            with ar.seeds(bad):
                ar.sample(partial, aux, cond=cond, keep_mask=ones)
    # a usable call after the refusals: everything kept, nothing drawn
    assert torch.equal(ar.sample(partial, aux, cond=cond, keep_mask=ones, temperature=torch.ones(B)), partial)
    # at the ABI
    T, k, p = [1.0] * B, [10] * (B * 4), [0.9] * (B * 4)
    assert P.c_sample_rows(nat, ar, aux, partial, cond, T, k, p)[0] == 0
    for null in ('T', 'k', 'p', 'partial', 'out'):
        rc, msg = P.c_sample_rows(nat, ar, aux, partial, cond, T, k, p, null=(null,))
        assert rc == -1 and b'null' in msg, null
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        rc, msg = P.c_sample_rows(nat, ar, aux, partial, cond, T[:-1] + [bad], k, p)
        assert rc == -1 and b'temperature' in msg, bad
    for bad in (float('nan'), float('inf')):
        rc, msg = P.c_sample_rows(nat, ar, aux, partial, cond, T, k, p, scale=[1.0] * (B - 1) + [bad])
        assert rc == -1 and b'finite' in msg, bad
    assert P.c_sample_rows(nat, ar, aux, partial, cond, T, k, p, scale=[2.0] * B)[0] == 0
    L = nat.lib()
    z = torch.zeros((2, 8))
    assert L.rqamd_sample_logits_rows(nat.ptr(z), 2, 8, None, None, None, None, 0, 0, None, None, None, None) == -1
