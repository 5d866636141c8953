"""Shared by tests/test_emu_composed_guidance.py (host emulator) and tests/test_gpu_composed_guidance.py (MI355X): the checks of composed
guidance -- RQTransformer.extra_conds / sample_guided(negative=...) over rqamd_rqt_sample_compose, and rqamd_compose_logits.  Models,
conditionings, seeds and the few-position mask come from tests/masked_sampling_cases.py and tests/guided_sampling_cases.py.  A composed
call runs the engine over (2 + K) B rows (images under `cond`, their twins under `uncond`, then K blocks under the extra conditionings),
so the engine's stepped teacher-forced logits over the same rows go through the kernels its sampling steps used, and apart from the
fp64 comparison of compose_logits every comparison is exact."""
import numpy as np
import torch

import guided_sampling_cases as G
import masked_sampling_cases as M

WEIGHTS = (-2.0, -0.5, 0.0, 0.75, 3.0)
KS = (1, 2, 4)


def extras_for(cfg, cond, K):
    """K conditionings that differ from `cond`, from uncond_for(cond) and from each other in every entry"""
    vc = max(cfg['vocab_size_cond'], 1)
    assert max(vc // 2, 1) > K                # (uncond_for adds vc // 2)
    u = G.uncond_for(cfg, cond)
    out = [(cond + 1 + k) % vc for k in range(K)]
    for e in out:
        assert bool((e != cond).all()) and bool((e != u).all())
    return out


# ------------------------------------------------------------------------------------------------ 1. compose_logits against fp64
def compose_inputs(rows, V, K, seed, device):
    """guide_inputs (N(0, 2) logits, a block of -inf columns) plus K extra rows with the same block, and weights drawn per row from WEIGHTS"""
    c, u, lo = G.guide_inputs(rows, V, seed, device)
    rng = np.random.default_rng(seed + 17)
    x = (2.0 * rng.standard_normal((K, rows, V))).astype(np.float32)
    x[:, :, lo:] = -np.inf
    w = rng.choice(np.asarray(WEIGHTS, dtype=np.float32), size=(K, rows))
    return c, u, torch.from_numpy(x).to(device), torch.from_numpy(w).to(device), lo


def check_compose_logits(nat, rows, V, device, seed=0):
    """g = rqamd_compose_logits against G = u + s (c - u) + E, E = sum_k w_k (x_k - u), in fp64.  With eps = 2**-24 and
    A = sum_k |w_k| |x_k - u| the bound per element is

        |g - G| <= 2 eps [ |G| + |c| + |E| + (K + 1) A + |s - 1| (|c - u| + |c| + |u| + 2 |E|) ]

    from the operations of compose_pair / guide_logit in their order: e carries one rounding per x_k - u (|w_k| |x_k - u| eps each, A eps in
    all) and one per fmaf of the chain (each at most A eps: K A eps), (K + 1) A eps together, and enters g through c' once -- in c' - u' it
    cancels; c' = fl(c + e) and u' = fl(u + e) round once each, (|c| + |E|) eps and (|u| + |E|) eps, the first reaching g directly and both
    through (s - 1)(c' - u'); c' - u' rounds once, |c - u| eps times |s - 1|; the final fmaf rounds once, |G| eps.  The factor 2 covers the
    second-order terms and the fp32 rounding of s - 1.  Rows whose e is 0 keep the pair and are inside the bound a fortiori.
    No NaN; the -inf columns stay -inf.  All weights 0, and every extra row equal to u: bit-equal to guide_logits(c, u, s)."""
    eps = 2.0 ** -24
    worst = 0.0
    for K in KS:
        c, u, x, w, lo = compose_inputs(rows, V, K, seed + K, device)
        c64, u64 = c.cpu().numpy().astype(np.float64)[:, :lo], u.cpu().numpy().astype(np.float64)[:, :lo]
        x64, w64 = x.cpu().numpy().astype(np.float64)[:, :, :lo], w.cpu().numpy().astype(np.float64)[:, :, None]
        E = (w64 * (x64 - u64)).sum(0)
        A = (np.abs(w64) * np.abs(x64 - u64)).sum(0)
        for s in G.SCALES:
            g = nat.compose_logits(c, u, x, w, s).cpu().numpy()
            assert g.shape == (rows, V) and g.dtype == np.float32
            assert not np.isnan(g).any(), (K, s)
            assert np.all(np.isneginf(g[:, lo:])) and np.all(np.isfinite(g[:, :lo])), (K, s)
            G64 = u64 + s * (c64 - u64) + E
            bound = 2.0 * eps * (np.abs(G64) + np.abs(c64) + np.abs(E) + (K + 1) * A
                                 + abs(s - 1.0) * (np.abs(c64 - u64) + np.abs(c64) + np.abs(u64) + 2.0 * np.abs(E)))
            err = np.abs(g[:, :lo].astype(np.float64) - G64)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), (K, s, float(err.max()), float((err / bound).max()))
            plain = nat.guide_logits(c, u, s).cpu().numpy().view(np.uint32)
            zero = nat.compose_logits(c, u, x, torch.zeros_like(w), s).cpu().numpy()
            assert np.array_equal(zero.view(np.uint32), plain), ('all weights zero', K, s)
            same = nat.compose_logits(c, u, u[None].expand(K, rows, V).contiguous(), torch.full_like(w, 3.0), s).cpu().numpy()
            assert np.array_equal(same.view(np.uint32), plain), ('extras equal to uncond', K, s)
    print(f'compose_logits ({rows}, {V}): largest error / bound over K in {KS} and {len(G.SCALES)} scales {worst:.3f}')
    return worst


def check_negative_zero(nat, device):
    """the e == 0 rule keeps a -0.0 logit: c + 0.0f would return +0.0"""
    c = torch.tensor([[-0.0, 1.0, -0.0, 2.0, -0.0]], dtype=torch.float32, device=device)
    u = torch.tensor([[0.5, -0.0, -0.0, 1.0, 3.0]], dtype=torch.float32, device=device)
    w = torch.tensor([[0.0]], dtype=torch.float32, device=device)
    got = nat.compose_logits(c, u, (u + 1.0)[None].contiguous(), w, 1.0).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, nat.guide_logits(c, u, 1.0).cpu().numpy().view(np.uint32))
    assert got[0, 0] == 0x80000000 and got[0, 4] == 0x80000000          # (c' = c + 0.0f = +0.0 would give fmaf(0, c' - u, c') = +0.0 here)


# ------------------------------------------------------------------------------------------------ 2. identity with zero weights
def check_zero_weight_identity(ar, aux, partial, cond, uncond, extras, seed, keep_mask=None, **kw):
    """sample_guided(s = 1) inside extra_conds(weights all 0) == the first B rows of sample over the (2 + K) B rows (partial repeated,
    cond = cat(cond, uncond, extras)): the same rows, Philox counters and kernels; e == 0 keeps the pair and guide() at s = 1 returns c"""
    B, n = partial.shape[0], 2 + len(extras)
    km = {} if keep_mask is None else dict(keep_mask=keep_mask)
    kmn = {} if keep_mask is None else dict(keep_mask=torch.cat([keep_mask] * n))
    M.seed_all(seed)
    with ar.extra_conds(conds=extras, weights=[0.0] * len(extras)):
        got = ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=1.0, **km, **kw)
    M.seed_all(seed)
    want = ar.sample(torch.cat([partial] * n), aux, cond=torch.cat([cond, uncond] + list(extras)), **kmn, **kw)
    assert got.shape == partial.shape and got.dtype == torch.int64
    assert torch.equal(got, want[:B]), ('composed call with zero weights at s = 1 differs from the plain call over (2 + K) B rows', len(extras), kw)
    return got


# ------------------------------------------------------------------------------------------------ 3. pairing
def stepped_logits(ar, aux, xs, conds, amp=False):
    """ONE stepped teacher-forced pass over len(conds) blocks of xs, LogitMask applied: (len(conds) * B, H, W, D, V)"""
    eng, cbs = ar._eng(amp), ar._checked_codebooks(aux)
    L = ar._on_side_stream(xs.device, lambda: eng.logits(torch.cat([xs] * len(conds)).contiguous(), torch.cat(list(conds)).contiguous(), cbs))
    for d, v in enumerate(ar.vocab_size):
        L[..., d, v:] = float('-inf')
    return L


def check_equal_rows_equal_logits(ar, aux, xs, cond, uncond):
    """what the pairing test rests on: equal input rows of one launch give equal logits, bit for bit"""
    B = xs.shape[0]
    L = stepped_logits(ar, aux, xs, [cond, uncond, uncond])
    return torch.equal(L[B:2 * B].view(torch.int32), L[2 * B:].view(torch.int32))


def check_pairing(ar, aux, partial, cond, uncond, seed, keep_mask=None, **kw):
    """K = 1 with the extra conditioning equal to `uncond`, s = 3: row 2B + b has the inputs of row B + b in the same launches, x - u is
    exactly 0, e == 0 keeps the pair -- the call with weight 5 returns the codes of the call with weight 0.  A fold that pairs rows
    wrongly, or a block that did not receive the drawn codes, breaks it."""
    km = {} if keep_mask is None else dict(keep_mask=keep_mask)
    out = []
    for w in (0.0, 5.0):
        M.seed_all(seed)
        with ar.extra_conds(conds=[uncond], weights=[w]):
            out.append(ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=3.0, **km, **kw))
    assert torch.equal(out[0], out[1]), 'an extra condition equal to uncond changed the codes'
    return out[0]


# ------------------------------------------------------------------------------------------------ 4. greedy / support
def composed_step_logits(nat, ar, aux, xs, cond, uncond, extras, weights, scale, amp=False):
    """compose_logits over the blocks of ONE stepped teacher-forced pass over the (2 + K) B rows: (B, H, W, D, V).  weights: K numbers or
    (B,) tensors"""
    B, K = xs.shape[0], len(extras)
    L = stepped_logits(ar, aux, xs, [cond, uncond] + list(extras), amp)
    V = L.shape[-1]
    per = L[0].numel() // V
    W = torch.stack([torch.as_tensor(w, dtype=torch.float32).reshape(-1).expand(B) if torch.is_tensor(w) else torch.full((B,), float(w)) for w in weights])
    W = W.to(xs.device).repeat_interleave(per, dim=1).contiguous()
    g = nat.compose_logits(L[:B].reshape(-1, V).contiguous(), L[B:2 * B].reshape(-1, V).contiguous(), L[2 * B:].reshape(K, -1, V).contiguous(), W, scale)
    return g.view(B, *L.shape[1:])


def check_composed_support(nat, ar, aux, xs, cond, uncond, extras, weights, scale, top_k, drawn=None, amp=False):
    """top_k = 1: every drawn code IS the argmax of the composed logits of its step (steps whose top-2 gap is exactly 0 are skipped, at most
    2 of them); otherwise its composed logit is at least the top_k-th largest of its row"""
    g = composed_step_logits(nat, ar, aux, xs, cond, uncond, extras, weights, scale, amp)
    drawn = torch.ones(xs.shape, dtype=torch.bool, device=xs.device) if drawn is None else drawn.to(xs.device)
    if top_k == 1:
        top2 = torch.topk(g, 2, dim=-1).values
        clear = (top2[..., 0] > top2[..., 1]) & drawn
        assert int(clear.sum()) >= int(drawn.sum()) - 2
        bad = clear & (xs != g.argmax(dim=-1))
        assert not bool(bad.any()), f'{int(bad.sum())} of {int(clear.sum())} greedy codes are not the argmax of the composed logits'
    else:
        mine = torch.gather(g, -1, xs[..., None])[..., 0]
        bad = drawn & ~(mine >= M.kth_largest(g, top_k))
        assert not bool(bad.any()), f'{int(bad.sum())} drawn codes outside the top-{top_k} of their composed row'
    return g


# ------------------------------------------------------------------------------------------------ 7. composition with the other forms
def check_composed_replay(ar, aux, partial, cond, uncond, extras, weights, scale, seed, mask_seed, first_keep=None, start_loc=(0, 0), **kw):
    """check_guided_replay inside extra_conds: a second composed call, same generator state, that keeps a random half of what the first
    call drew and is given an out-of-range filler elsewhere returns the first call's codes, bit for bit"""
    with ar.extra_conds(conds=extras, weights=weights):
        return G.check_guided_replay(ar, aux, partial, cond, uncond, scale, seed, mask_seed, first_keep=first_keep, start_loc=start_loc, **kw)


def check_per_image_weights(ar, aux, partial, cond, uncond, extra, weights, seeds, keep_mask=None, **kw):
    """a (B,) weight tensor gives image b the codes of the scalar call with b's weight, under seeds()"""
    km = {} if keep_mask is None else dict(keep_mask=keep_mask)
    dev = partial.device
    with ar.seeds(seeds):
        with ar.extra_conds(conds=[extra], weights=[torch.tensor(weights, dtype=torch.float32, device=dev)]):
            got = ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=3.0, **km, **kw)
        rows = []
        for b, w in enumerate(weights):
            with ar.extra_conds(conds=[extra], weights=[float(w)]):
                rows.append(ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=3.0, **km, **kw)[b])
    for b in range(len(weights)):
        assert torch.equal(got[b], rows[b]), f'image {b} of the per-image call differs from the scalar call with its weight'
    assert len({tuple(r.reshape(-1).tolist()) for r in rows}) > 1 or len(set(weights)) == 1
    return got


def check_log_probs(nat, ar, aux, partial, cond, uncond, extras, weights, seeds, keep_mask=None, top_k=50, top_p=0.9, scale=3.0):
    """return_log_probs() inside extra_conds(), under seeds(): the codes are those of the call outside return_log_probs(); `draw` equals,
    bit for bit, the log-probability rqamd_sample_logits_logp returns for the composed logits of the step (compose_logits over the blocks
    of the stepped pass), drawn with image b's Philox key and the step's counter -- which also draws the code; `model` is bit-equal to
    the `model` of the zero-weight call wherever the codes of the two calls agree up to and including the slot.  -> number of such slots"""
    B, dev = partial.shape[0], partial.device
    (H, W, D) = ar.block_size
    km = {} if keep_mask is None else dict(keep_mask=keep_mask)
    kw = dict(cond=cond, uncond=uncond, guidance_scale=scale, top_k=top_k, top_p=top_p, **km)
    with ar.seeds(seeds):
        with ar.extra_conds(conds=extras, weights=weights):
            plain = ar.sample_guided(partial, aux, **kw)
            with ar.return_log_probs():
                codes, lp = ar.sample_guided(partial, aux, **kw)
        with ar.extra_conds(conds=extras, weights=[0.0] * len(extras)), ar.return_log_probs():
            codes0, lp0 = ar.sample_guided(partial, aux, **kw)
    assert torch.equal(codes, plain), 'the armed composed call drew other codes'
    assert lp.model_uncond is not None and lp.draw.shape == codes.shape
    drawn = torch.ones(codes.shape, dtype=torch.bool, device=dev) if keep_mask is None else ~keep_mask.to(dev)
    g = composed_step_logits(nat, ar, aux, codes, cond, uncond, extras, weights, scale)
    sd = torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64, device=dev)
    T = torch.ones((B,), dtype=torch.float32, device=dev)
    Kt = torch.full((B,), top_k, dtype=torch.int32, device=dev)
    Pt = torch.full((B,), top_p, dtype=torch.float32, device=dev)
    n = 0
    for pos in range(H * W):
        h, w = divmod(pos, W)
        for d in range(D):
            dr = drawn[:, h, w, d]
            if not bool(dr.any()):
                continue
            smp, lg = nat.sample_logits_logp(g[:, h, w, d].contiguous(), row_temperature=T, row_top_k=Kt, row_top_p=Pt, row_seeds=sd, offset=pos * D + d)
            assert torch.equal(smp[dr], codes[:, h, w, d][dr]), (pos, d, 'the stand-alone sampler draws another code from the composed logits')
            assert torch.equal(lg[dr].view(torch.int32), lp.draw[:, h, w, d][dr].view(torch.int32)), (pos, d, 'draw differs from the stand-alone log-probability')
            n += int(dr.sum())
    assert n == int(drawn.sum())
    agree = (codes == codes0).view(B, -1).cpu()
    prefix = torch.cumprod(agree.to(torch.int64), dim=1).bool()          # codes agree at every slot up to and including this one
    m, m0 = lp.model.view(B, -1).cpu(), lp0.model.view(B, -1).cpu()
    ran = ~torch.isnan(m0)
    assert torch.equal(torch.isnan(m), torch.isnan(m0))
    sel = prefix & ran
    assert torch.equal(m[sel].view(torch.int32), m0[sel].view(torch.int32)), 'model log-probabilities are not those of the raw conditional logits'
    print(f'composed log-probabilities: {n} draws re-derived exactly; model compared at {int(sel.sum())} slots')
    return int(sel.sum())
