"""Shared by tests/test_emu_guided_sampling.py (host emulator) and tests/test_gpu_guided_sampling.py (MI355X): the checks of
RQTransformer.sample_guided / rqamd_rqt_sample_guided / rqamd_guide_logits.  Models, conditionings and seeds come from
tests/masked_sampling_cases.py.  Apart from the fp64 comparison of guide_logits every comparison is exact: a guided call runs the
engine over 2B rows (images under `cond`, then their twins under `uncond`), so the engine's stepped teacher-forced logits over
cat(xs, xs) / cat(cond, uncond) go through the kernels its sampling steps used."""
import numpy as np
import torch

import masked_sampling_cases as M

SCALES = (0.0, 1.0, 1.5, 3.0, 7.5)
# all three sampler kernels draw: unfiltered (streaming), top-k + top-p (register kernel, then the general one), and a per-depth mix
# in which depth 1 takes the register kernel alone, depth 2 the general kernel alone (top-k covers the vocabulary) and depth 3 none
SAMPLERS = (dict(), dict(top_k=50, top_p=0.9), dict(top_k=[50, 50, 500, 500], top_p=[0.9, 1.0, 0.9, 1.0]))


def uncond_for(cfg, cond):
    """a conditioning that differs from `cond` in every entry"""
    vc = max(cfg['vocab_size_cond'], 1)
    assert vc > 1
    return (cond + max(vc // 2, 1)) % vc


def few_mask(B, H=4, W=4, D=4):
    """keep everything but: position 0, depths 2.. of row 0 only; position 1, every depth of every row; position 2, depths 0 and 1 of
    every row.  Three positions run, nothing after them (the emulator needs minutes for a full pass)."""
    keep = torch.ones((B, H * W, D), dtype=torch.bool)
    keep[0, 0, 2:] = False
    keep[:, 1, :] = False
    keep[:, 2, :2] = False
    return keep.view(B, H, W, D)


def random_codes(shape, vocab, seed, device):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, vocab, shape)).to(device)


# ------------------------------------------------------------------------------------------------ guide_logits against fp64
def guide_inputs(rows, V, seed, device):
    """N(0, 2) logits, a block of columns at -inf in both inputs (what LogitMask leaves)"""
    rng = np.random.default_rng(seed)
    c = (2.0 * rng.standard_normal((rows, V))).astype(np.float32)
    u = (2.0 * rng.standard_normal((rows, V))).astype(np.float32)
    lo = V - max(V // 5, 1)
    c[:, lo:] = -np.inf
    u[:, lo:] = -np.inf
    return torch.from_numpy(c).to(device), torch.from_numpy(u).to(device), lo


def check_guide_logits(nat, rows, V, device, seed=0):
    """|g - g64| <= 2**-23 (|c| + |s - 1| |c - u|) per element: one rounding of c - u (relative 2**-24, times |s - 1|) plus the one
    rounding of the fmaf (relative 2**-24 of a result no larger than |c| + |s - 1| |c - u|) -- half of the bound each, with room
    for the fp32 rounding of s - 1 itself.  s = 1: bit-equal to c.  -inf columns stay -inf; no NaN."""
    c, u, lo = guide_inputs(rows, V, seed, device)
    c64, u64 = c.cpu().numpy().astype(np.float64), u.cpu().numpy().astype(np.float64)
    worst = 0.0
    for s in SCALES:
        g = nat.guide_logits(c, u, s).cpu().numpy()
        assert g.shape == (rows, V) and g.dtype == np.float32
        assert not np.isnan(g).any(), s
        assert np.all(np.isneginf(g[:, lo:])) and np.all(np.isfinite(g[:, :lo])), s
        g64 = c64[:, :lo] + (s - 1.0) * (c64[:, :lo] - u64[:, :lo])
        bound = 2.0 ** -23 * (np.abs(c64[:, :lo]) + abs(s - 1.0) * np.abs(c64[:, :lo] - u64[:, :lo]))
        err = np.abs(g[:, :lo].astype(np.float64) - g64)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (s, float(err.max()))
        if s == 1.0:
            assert np.array_equal(g.view(np.uint32), c.cpu().numpy().view(np.uint32))
    print(f'guide_logits ({rows}, {V}): largest error / bound over {len(SCALES)} scales {worst:.3f}')


# ------------------------------------------------------------------------------------------------ s = 1 identity
def check_s1_identity(ar, aux, partial, cond, uncond, seed, keep_mask=None, **kw):
    """sample_guided(s = 1) == sample over the 2B rows (partial twice, cond then uncond), first half: the same row indices, Philox
    counters and 2B-row kernels; at s = 1 guide() returns the conditional logit bit for bit.  (A mask is given to both calls, for all
    2B rows of the plain one: row b of it depends on row b's codes alone.)"""
    B = partial.shape[0]
    km = {} if keep_mask is None else dict(keep_mask=keep_mask)
    km2 = {} if keep_mask is None else dict(keep_mask=torch.cat([keep_mask, keep_mask]))
    M.seed_all(seed)
    got = ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=1.0, **km, **kw)
    M.seed_all(seed)
    want = ar.sample(torch.cat([partial, partial]), aux, cond=torch.cat([cond, uncond]), **km2, **kw)
    assert got.shape == partial.shape and got.dtype == torch.int64
    assert torch.equal(got, want[:B]), ('guided call at s = 1 differs from the plain call over 2B rows', kw)
    if keep_mask is None:
        assert not torch.equal(want[:B], want[B:])                  # the twins of the plain call do draw something else
    return got


# ------------------------------------------------------------------------------------------------ greedy / support
def guided_step_logits(nat, ar, aux, xs, cond, uncond, scale, amp=False):
    """guide_logits of the two halves of ONE stepped teacher-forced pass over cat(xs, xs) / cat(cond, uncond), LogitMask applied:
    (B, H, W, D, V)"""
    B = xs.shape[0]
    eng, cbs = ar._eng(amp), ar._checked_codebooks(aux)
    L = ar._on_side_stream(xs.device, lambda: eng.logits(torch.cat([xs, xs]).contiguous(), torch.cat([cond, uncond]).contiguous(), cbs))
    for d, v in enumerate(ar.vocab_size):
        L[..., d, v:] = float('-inf')
    V = L.shape[-1]
    g = nat.guide_logits(L[:B].reshape(-1, V).contiguous(), L[B:].reshape(-1, V).contiguous(), scale)
    return g.view(B, *L.shape[1:])


def check_guided_support(nat, ar, aux, xs, cond, uncond, scale, top_k, drawn=None, amp=False):
    """top_k = 1: every drawn code IS the argmax of the guided logits of its step (steps whose top-2 gap is exactly 0 are skipped);
    otherwise its guided logit is at least the top_k-th largest of its row.  Catches a twin that did not receive the drawn codes, a
    wrong pairing and a wrong scale."""
    g = guided_step_logits(nat, ar, aux, xs, cond, uncond, scale, amp)
    drawn = torch.ones(xs.shape, dtype=torch.bool, device=xs.device) if drawn is None else drawn.to(xs.device)
    if top_k == 1:
        top2 = torch.topk(g, 2, dim=-1).values
        clear = (top2[..., 0] > top2[..., 1]) & drawn
        assert int(clear.sum()) >= int(drawn.sum()) - 2
        bad = clear & (xs != g.argmax(dim=-1))
        assert not bool(bad.any()), f'{int(bad.sum())} of {int(clear.sum())} greedy codes are not the argmax of the guided logits'
    else:
        mine = torch.gather(g, -1, xs[..., None])[..., 0]
        bad = drawn & ~(mine >= M.kth_largest(g, top_k))
        assert not bool(bad.any()), f'{int(bad.sum())} drawn codes outside the top-{top_k} of their guided row'


# ------------------------------------------------------------------------------------------------ guided + masked replay
def check_guided_replay(ar, aux, partial, cond, uncond, scale, seed, mask_seed, first_keep=None, start_loc=(0, 0), **kw):
    """codes0 = a guided call; a second guided call, same generator state, that keeps a random half of what the first call drew (and
    whatever the first call kept) and is given an out-of-range filler elsewhere must return codes0, bit for bit"""
    dev = partial.device
    k1 = {} if first_keep is None else dict(keep_mask=first_keep)
    M.seed_all(seed)
    codes0 = ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=scale, start_loc=start_loc, **k1, **kw)
    half = torch.from_numpy(np.random.default_rng(mask_seed).random(tuple(partial.shape)) < 0.5).to(dev)
    keep = half if first_keep is None else (half | first_keep.to(dev))
    given = torch.where(keep, codes0, torch.full_like(codes0, M.OUT_OF_RANGE))
    (B, H, W, D) = partial.shape
    start = start_loc[0] * W + start_loc[1]
    given.view(B, H * W, D)[:, :start] = partial.view(B, H * W, D)[:, :start]        # (the prefix before start_loc is kept by the call itself)
    M.seed_all(seed)
    out = ar.sample_guided(given, aux, cond=cond, uncond=uncond, guidance_scale=scale, start_loc=start_loc, keep_mask=keep, **kw)
    assert torch.equal(out, codes0), ('masked guided draw differs from the guided draw', kw)
    return codes0
