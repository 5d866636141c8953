"""Shared by tests/test_emu_anchored_sampling.py (host emulator) and tests/test_gpu_anchored_sampling.py (MI355X): the checks of anchored
sampling -- RQTransformer.anchor over rqamd_rqt_sample_anchor, and rqamd_anchor_logits.  The tiny model (4 x 4 x 4, V = 500, dim = 64), the
quantiser with the fixture's codebook and the first two feature maps come from tests/soft_loss_cases.py, conditionings, seeds, samplers and
masks from tests/masked_sampling_cases.py / tests/guided_sampling_cases.py.  The host loop (``cached=False``) steps the engine over the
same rows and folds the anchor in through rqamd_anchor_logits, the kernels and the device function of the engine's own three launches, so
apart from the fp64 comparison of the fold every comparison is exact."""
import numpy as np
import torch

from oracle import configs as C

import guided_sampling_cases as G
import masked_sampling_cases as M
import soft_loss_cases as S

WEIGHT_SET = (0.0, 0.25, 1.0, 8.0)
PER_DEPTH = (8.0, 2.0, 0.5, 0.0)


def setup(dev, B, cfg=C.RQT_TINY):
    """(model, model_aux with a real quantiser, cond, z (B, 4, 4, 64): the fixture's two feature maps, then seeded ones of the same scale)"""
    ar, aux = S.model(cfg, dev), S.Aux(S.codebook(), dev)
    more = (0.15 * np.random.default_rng(S.Z_SEED + 1).standard_normal((max(B - 2, 0), 4, 4, 64))).astype(np.float32)
    z = torch.from_numpy(np.concatenate([S.features(), more])[:B]).to(dev)
    return ar, aux, M.cond_for(cfg, B, dev), z


def image_table(B, seed=3, H=4, W=4, D=4):
    """a (B, H, W, D) weight table over WEIGHT_SET with zeros in it: whole positions, one image's depth, and single slots"""
    w = np.random.default_rng(seed).choice(np.asarray(WEIGHT_SET, dtype=np.float32), size=(B, H * W, D))
    w[:, 1] = 0.0
    w[0, :, 2] = 0.0
    w[B - 1, 2, 0] = 0.0
    assert (w == 0).any() and (w > 0).any()
    return torch.from_numpy(w.reshape(B, H, W, D))


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. anchor_logits alone
def anchor_inputs(nat, rows, V, dim, d, seed, device):
    rng = np.random.default_rng(seed)
    c, u, lo = G.guide_inputs(rows, V, seed, device)
    cbs = [torch.from_numpy((0.1 * rng.standard_normal((V, dim))).astype(np.float32)).to(device) for _ in range(d + 1)]
    norms = [nat.rq_code_norms(cb) for cb in cbs]
    z = torch.from_numpy((0.15 * rng.standard_normal((rows, dim))).astype(np.float32)).to(device)
    codes = torch.from_numpy(rng.integers(0, V, (rows, d))).to(device)
    w = torch.from_numpy(rng.choice(np.asarray(WEIGHT_SET, dtype=np.float32), size=(rows,))).to(device)
    return c, u, lo, cbs, norms, z, codes, w


def check_anchor_logits(nat, rows, V, dim, d, device, seed=0):
    """rqamd_anchor_logits over (rows, V, dim) at depth d: resid_out bit-equal to the numpy fp32 sequential subtraction; dist_out bit-equal
    to rqamd_rq_distances of that residual over the same rows; out against fp64 G = l - w * dist taken from the fp32 dist_out, with
    |g - G| <= 2 * 2**-24 * |G| + 2**-149 (one fmaf: one rounding of the exact result, relative 2**-24, or an absolute 2**-149 in the
    subnormal range; the factor 2 as in check_compose_logits) -- derived, not measured; the -inf columns stay -inf and nothing is NaN; rows
    with w = 0 (a hand-made row of -0.0 logits among them) and rows whose z holds a NaN or an inf are bit-equal to the input; the guided
    form is bit-equal to two unguided calls.  -> largest error / bound"""
    c, u, lo, cbs, norms, z, codes, w = anchor_inputs(nat, rows, V, dim, d, seed, device)
    cases = []
    if rows >= 5:                                          # one call: a zero-weight row of -0.0 logits, a NaN row, an inf row, drawn weights
        w[0] = 0.0
        c[0, :lo] = -0.0
        w[1] = w[2] = 8.0
        z[1, 5] = float('nan')
        z[2, dim - 3] = float('inf')
        w[3], w[4] = 1.0, 0.25
        cases.append((z, w))
    else:                                                  # few rows: every weight and the drawn ones, then a NaN and an inf in z, a call each
        cases.append((z, w))
        for wv in WEIGHT_SET:
            cases.append((z, torch.full_like(w, wv)))
        for bad in (float('nan'), float('-inf')):
            zb = z.clone()
            zb[0, 5] = bad
            cases.append((zb, torch.full_like(w, 8.0)))
        c[0, 0] = -0.0
    worst, eps = 0.0, 2.0 ** -24
    cb_np = [cb.cpu().numpy() for cb in cbs]
    for zc, wc in cases:
        out, resid, dist = nat.anchor_logits(c, zc, codes, cbs, norms, wc, want_resid=True, want_dist=True)
        assert out.shape == (rows, V) and out.dtype == torch.float32 and resid.shape == (rows, dim) and dist.shape == (rows, V)
        # residual: the quantiser's order, in fp32
        r = zc.cpu().numpy().copy()
        for j in range(d):
            r = r - cb_np[j][codes[:, j].cpu().numpy()]
        assert r.dtype == np.float32
        finite = np.isfinite(zc.cpu().numpy()).all(axis=1)
        got_r = resid.cpu().numpy()
        assert np.array_equal(got_r[finite].view(np.uint32), r[finite].view(np.uint32)), 'residual differs from the fp32 sequential subtraction'
        assert np.array_equal(got_r[~finite], r[~finite], equal_nan=True)
        # distances: the quantiser's kernel over the same rows
        want_d = nat.rq_distances(resid, cbs[d], norms[d])
        assert torch.equal(bits(dist), bits(want_d)), 'distances differ from rq_distances over the same rows'
        # the fold
        g, l, dd, wn = out.cpu().numpy(), c.cpu().numpy(), dist.cpu().numpy(), wc.cpu().numpy()
        assert not np.isnan(g).any()
        assert np.all(np.isneginf(g[:, lo:])) and np.all(np.isfinite(g[:, :lo]))
        same = (wn == 0) | ~finite
        assert np.array_equal(g[same].view(np.uint32), l[same].view(np.uint32)), 'a row with w = 0 or a non-finite z changed'
        assert np.all(np.isfinite(dd[finite]))
        act = ~same
        if act.any():
            G64 = l[act, :lo].astype(np.float64) - wn[act, None].astype(np.float64) * dd[act, :lo].astype(np.float64)
            err = np.abs(g[act, :lo].astype(np.float64) - G64)
            bound = 2.0 * eps * np.abs(G64) + 2.0 ** -149
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (rows, V, dim, d, float(err.max()), float((err / bound).max()))
            assert not np.array_equal(g[act], l[act])
        # guided form == two unguided calls
        oc, ou = nat.anchor_logits(c, zc, codes, cbs, norms, wc, logits_u=u)
        assert torch.equal(bits(oc), bits(out)), 'guided form, conditional half'
        assert torch.equal(bits(ou), bits(nat.anchor_logits(u, zc, codes, cbs, norms, wc))), 'guided form, unconditional half'
    assert worst > 0.0                                     # (some row went through the fmaf)
    if rows < 5:
        assert np.signbit(nat.anchor_logits(c, z, codes, cbs, norms, torch.zeros_like(w)).cpu().numpy()[0, 0])
    print(f'anchor_logits ({rows}, {V}, {dim}) depth {d}: largest error / bound {worst:.3f}')
    return worst


# ------------------------------------------------------------------------------------------------ 2. zero weight is the plain call
def same_result(a, b):
    if isinstance(a, tuple):
        (ca, la), (cb, lb) = a, b
        ok = torch.equal(ca, cb)
        for x, y in zip(la, lb):
            ok = ok and ((x is None and y is None) or torch.equal(bits(x), bits(y)))
        return ok
    return torch.equal(a, b)


def check_zero_weight(ar, z, run, seed, weight=0.0):
    """`run()` -- any sampling call -- inside anchor(z, 0) returns what it returns outside, bit for bit (log-probabilities included)"""
    M.seed_all(seed)
    want = run()
    M.seed_all(seed)
    with ar.anchor(z, weight):
        got = run()
    assert same_result(got, want), 'a zero-weight anchor changed the result'
    M.seed_all(seed)
    with ar.anchor(None):
        assert same_result(run(), want)
    return want


# ------------------------------------------------------------------------------------------------ 3. engine == host loop
def check_host_loop(ar, z, weight, run, seed, differs_from=None):
    """inside anchor(z, weight): `run(cached=True)` (the engine) == `run(cached=False)` (the host loop over anchor_logits), bit for bit"""
    with ar.anchor(z, weight):
        M.seed_all(seed)
        a = run(cached=True)
        M.seed_all(seed)
        b = run(cached=False)
    assert a.dtype == torch.int64 and torch.equal(a, b), 'the engine and the host loop drew different codes'
    if differs_from is not None:
        assert not torch.equal(a, differs_from), 'the anchor did not change the codes'
    return a


def stepped_logits(ar, aux, xs, cond, amp=False):
    """ONE stepped teacher-forced pass over xs, LogitMask applied: (B, H, W, D, V)"""
    eng, cbs = ar._eng(amp), ar._checked_codebooks(aux)
    L = ar._on_side_stream(xs.device, lambda: eng.logits(xs.contiguous(), cond, cbs))
    for d, v in enumerate(ar.vocab_size):
        L[..., d, v:] = float('-inf')
    return L


def anchored_step_logits(nat, ar, aux, xs, cond, z, wtab):
    """anchor_logits over every step of ONE stepped pass over the final codes xs: (B, H, W, D, V); wtab (B, H, W, D) on the device"""
    L = stepped_logits(ar, aux, xs, cond)
    q = aux.quantizer
    cbs, norms = q.codebook_list(), q._norm_list()
    (B, H, W, D) = xs.shape
    out = torch.empty_like(L)
    for h in range(H):
        for w in range(W):
            for d in range(D):
                out[:, h, w, d] = nat.anchor_logits(L[:, h, w, d].contiguous(), z[:, h, w], xs[:, h, w, :d], cbs, norms, wtab[:, h, w, d].contiguous())
    return L, out


def check_log_probs(nat, ar, aux, partial, cond, z, weight, wtab, seeds, top_k=50, top_p=0.9, drawn=None, keep_mask=None):
    """return_log_probs() inside anchor(), under seeds(): the codes are those of the call outside return_log_probs(); `draw` equals, bit
    for bit, the log-probability rqamd_sample_logits_logp returns for the anchored logits of the step (anchor_logits over the stepped
    pass), drawn with image b's Philox key and the step's counter -- which also draws the code: the host loop's draw.  `model` is the
    log-softmax of the stepped RAW logits at the drawn code: bit-equal to the `model` of an unanchored armed call that is given the
    anchored call's codes as kept codes -- the engine's own log-probability kernel over the raw logits of the same steps -- in every row
    but row 0 (which draws the last depth of every position so that every head runs) and at the first position of row 0."""
    B, dev = partial.shape[0], partial.device
    (H, W, D) = ar.block_size
    km = {} if keep_mask is None else dict(keep_mask=keep_mask)
    kw = dict(cond=cond, top_k=top_k, top_p=top_p, **km)
    with ar.seeds(seeds):
        with ar.anchor(z, weight):
            plain = ar.sample(partial, aux, **kw)
            with ar.return_log_probs():
                codes, lp = ar.sample(partial, aux, **kw)
        keep = torch.ones(codes.shape, dtype=torch.bool, device=dev)
        heads = torch.ones((H, W), dtype=torch.bool, device=dev) if keep_mask is None else (~keep_mask.to(dev)).any(dim=3).any(dim=0)
        keep[0, :, :, D - 1] = ~heads                      # row 0 draws the last depth wherever the anchored call ran a head
        with ar.return_log_probs():
            _, lp0 = ar.sample(codes, aux, cond=cond, top_k=top_k, top_p=top_p, keep_mask=keep)
    assert torch.equal(codes, plain), 'the armed anchored call drew other codes'
    assert lp.model_uncond is None and lp.draw.shape == codes.shape
    if drawn is None:
        drawn = torch.ones(codes.shape, dtype=torch.bool, device=dev) if keep_mask is None else ~keep_mask.to(dev)
    drawn = drawn.to(dev)
    _, g = anchored_step_logits(nat, ar, aux, codes, cond, z, wtab.to(dev))
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
            assert torch.equal(smp[dr], codes[:, h, w, d][dr]), (pos, d, 'the stand-alone sampler draws another code from the anchored logits')
            assert torch.equal(bits(lg[dr]), bits(lp.draw[:, h, w, d][dr])), (pos, d, 'draw differs from the stand-alone log-probability')
            n += int(dr.sum())
    assert n == int(drawn.sum())
    m, m0 = lp.model.view(B, H * W, D), lp0.model.view(B, H * W, D)
    ran = ~torch.isnan(m)
    assert bool(ran[1:].any()) and not bool(torch.isnan(m0[1:][ran[1:]]).any())
    assert torch.equal(bits(m[1:][ran[1:]]), bits(m0[1:][ran[1:]])), 'model is not the log-softmax of the raw logits'
    first = int(ran[0].any(dim=1).nonzero()[0])           # row 0: its first position with a head, before its own codes diverge
    assert torch.equal(bits(m[0, first, :D - 1]), bits(m0[0, first, :D - 1]))
    # and, independent of the engine's kernel, every row against fp64 log_softmax of the stepped RAW logits at the code: the bound of the
    # step form of log_prob_kernel at V = 500 (tests/sample_logp_cases.py: MODEL_BOUND), which this change does not touch
    import sample_logp_cases as LP
    raw = stepped_logits(ar, aux, codes, cond).double().view(B, H * W, D, -1)
    want = torch.gather(torch.log_softmax(raw, dim=-1), -1, codes.view(B, H * W, D, 1))[..., 0]
    err = float((m.double() - want)[ran].abs().max())
    assert err <= LP.MODEL_BOUND, f'model against fp64 log_softmax of the raw stepped logits: {err:.3e} > {LP.MODEL_BOUND:.3e}'
    anc = torch.gather(torch.log_softmax(g.double().view(B, H * W, D, -1), dim=-1), -1, codes.view(B, H * W, D, 1))[..., 0]
    assert float((want - anc)[ran].abs().max()) > 100 * LP.MODEL_BOUND      # (the anchored logits would have given other values)
    print(f'anchored log-probabilities: {n} draws re-derived exactly; model compared at {int(ran[1:].sum()) + D - 1} slots bit for bit, '
          f'at {int(ran.sum())} against fp64 (largest error {err:.3e})')
    return n


# ------------------------------------------------------------------------------------------------ 4. a strong anchor returns the image's codes
def strong_anchor_inputs(aux, B, seed, dev, H=4, W=4, D=4):
    """z = sum_d codebook[k0[..., d]] + 1e-3 N(0, 1) for seeded codes k0 (B, H, W, D), and k = the quantiser's codes of z.  (With one
    codebook shared by the depths the four summands are interchangeable: which of them is nearest to z, and so the greedy trajectory of
    the quantiser, is not k0 in its seeded order -- k is the trajectory a strong anchor must follow, "get_codes of the image".)"""
    rng = np.random.default_rng(seed)
    cb = aux.quantizer.codebook_list()[0].cpu().numpy()
    k0 = rng.integers(0, cb.shape[0], (B, H, W, D))
    z = cb[k0].sum(axis=3) + 1e-3 * rng.standard_normal((B, H, W, cb.shape[1]))
    z = torch.from_numpy(z.astype(np.float32)).to(dev)
    k = aux.quantizer.quantize(z)[1]
    assert k.shape == (B, H, W, D) and k.dtype == torch.int64
    return k, z


def check_strong_anchor(nat, ar, aux, cond, k, z, keep_mask=None):
    """The precondition, from quantities computed here: along the trajectory k, for every (b, p, d) at which a code is drawn,
        w * (second smallest distance - smallest distance) >= 2 * max |stepped logit| + 60
    with the distances of the residual r_d(b, p) of k (anchor_logits' dist_out) and the stepped raw logits of k, and the smallest distance
    at k[b, p, d]; w the smallest power of two for which it holds.  Any other code then has an anchored logit at least 60 below that of
    k, a probability below e**-60 each, below N * V * e**-60 in all: the anchored call returns k exactly, at temperature 1 without
    filters and with top_k = 1."""
    (B, H, W, D) = k.shape
    dev = k.device
    q = aux.quantizer
    cbs, norms = q.codebook_list(), q._norm_list()
    L = stepped_logits(ar, aux, k, cond)
    drawn = torch.ones(k.shape, dtype=torch.bool, device=dev) if keep_mask is None else ~keep_mask.to(dev)
    lmax = float(L[torch.isfinite(L)].abs().max())
    gap = float('inf')
    ones = torch.ones((B,), dtype=torch.float32, device=dev)
    for h in range(H):
        for w in range(W):
            for d in range(D):
                _, dist = nat.anchor_logits(L[:, h, w, d].contiguous(), z[:, h, w], k[:, h, w, :d], cbs, norms, ones, want_dist=True)
                two = torch.topk(dist, 2, dim=-1, largest=False)
                assert torch.equal(two.indices[:, 0], k[:, h, w, d]), 'the nearest code of the residual is not the trajectory code'
                sel = drawn[:, h, w, d]
                if bool(sel.any()):
                    gap = min(gap, float((two.values[:, 1] - two.values[:, 0])[sel].min()))
    assert gap > 0
    wt = 1.0
    while wt * gap < 2.0 * lmax + 60.0:
        wt *= 2.0
    assert wt * gap >= 2.0 * lmax + 60.0 and wt <= 2.0 ** 40
    print(f'strong anchor: smallest distance gap {gap:.4e}, largest |logit| {lmax:.3f}, w = {wt:g}')
    km = {} if keep_mask is None else dict(keep_mask=keep_mask)
    partial = k if keep_mask is not None else torch.zeros_like(k)
    for kw in (dict(), dict(top_k=1)):
        M.seed_all(11)
        with ar.anchor(z, wt):
            got = ar.sample(partial, aux, cond=cond, **km, **kw)
        assert torch.equal(got, k), ('a strong anchor did not return the image codes', kw, int((got != k).sum()))
    return wt


# ------------------------------------------------------------------------------------------------ 6. refusals
def check_refusals(ar, aux, cond, z, partial, usable, keep_mask=None):
    """each refused call raises the documented error before anything runs; `usable()` then checks a plain call against what it returned before"""
    import pytest
    B = partial.shape[0]
    km = {} if keep_mask is None else dict(keep_mask=keep_mask)
    kw = dict(cond=cond, top_k=50, **km)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='weight'):
            with ar.anchor(z, bad):
                ar.sample(partial, aux, **kw)
        tab = torch.ones((B, 4, 4, 4))
        tab[B - 1, 3, 3, 3] = bad
        with pytest.raises(ValueError, match='weight'):
            with ar.anchor(z, tab):
                ar.sample_guided(partial, aux, uncond=G.uncond_for(C.RQT_TINY, cond), guidance_scale=2.0, **kw)
        usable()
    with pytest.raises(ValueError, match='shape'):
        with ar.anchor(z, torch.ones((B + 1,))):
            ar.sample(partial, aux, **kw)
    with pytest.raises(ValueError, match='shape'):
        with ar.anchor(z[:, :3], 1.0):
            ar.sample(partial, aux, **kw)
    usable()
    with pytest.raises(NotImplementedError, match='dim'):
        with ar.anchor(z[..., :32], 1.0):
            ar.sample(partial, aux, **kw)
    usable()
    with pytest.raises(NotImplementedError, match='shared'):
        with ar.shared_cond(2), ar.anchor(z[:2], 1.0):      # (two images: one group of two)
            ar.sample(partial[:2], aux, cond=cond[:1], top_k=50, **({} if keep_mask is None else dict(keep_mask=keep_mask[:2])))
    with pytest.raises(NotImplementedError, match='extra_conds|compose'):
        with ar.extra_conds(conds=[cond], weights=[0.5]), ar.anchor(z, 1.0):
            ar.sample_guided(partial, aux, uncond=G.uncond_for(C.RQT_TINY, cond), guidance_scale=2.0, **kw)
    usable()
    ar.sampler = 'torch'
    try:
        with pytest.raises(NotImplementedError, match='torch'):
            with ar.anchor(z, 1.0):
                ar.sample(partial, aux, **kw)
    finally:
        ar.sampler = 'philox'
    usable()


def check_tuple_refused(dev, z):
    """RQT_TINY_TUPLE: depths with different vocabularies"""
    import pytest
    tup = S.model(C.RQT_TINY_TUPLE, dev)
    aux = S.Aux(S.codebook(), dev)
    zeros = torch.zeros((z.shape[0], 4, 4, 4), dtype=torch.long, device=dev)
    with pytest.raises(NotImplementedError, match='vocabular'):
        with tup.anchor(z, 1.0):
            tup.sample(zeros, aux)
    # and the engine's own check, behind the mirror: armed at the handle, refused by the armed call (RQAMD_ERR_UNSUPPORTED), which
    # consumes the arming -- the same call again is the plain call
    eng, cbs = tup._sampling_eng(False), tup._checked_codebooks(aux)
    q = aux.quantizer
    args = (zeros, None, cbs, (0, 0), 1.0, [50] * 4, [1.0] * 4, 2, 0, False)
    want = tup._on_side_stream(dev, lambda: eng.sample(*args))
    eng.arm_anchor(z, q.codebook_list(), q._norm_list(), [1.0] * 64, False)
    with pytest.raises(NotImplementedError, match='rqt_sample_anchor: depths with different vocabularies'):
        tup._on_side_stream(dev, lambda: eng.sample(*args))
    assert torch.equal(tup._on_side_stream(dev, lambda: eng.sample(*args)), want)


def check_abi_refusals(nat, ar, aux, cond, z, partial, keep8=None, active=None, sync=lambda: None):
    """at the ABI: the refusals of rqamd_rqt_sample_anchor are made by the armed call, before anything is enqueued, and each consumes the
    arming -- the same call made again is a plain call and returns the plain call's codes"""
    import ctypes
    from rqvae._native import _int_array, _ptr_array
    ptr = nat.ptr
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    q = aux.quantizer
    L, h = eng._L, eng._h
    D, B = 4, partial.shape[0]
    cb, tk, tp = _ptr_array(cbs[:D]), _int_array([50] * D), (ctypes.c_float * D)(*[1.0] * D)
    acb, acn = _ptr_array(q.codebook_list()[:D]), _ptr_array(q._norm_list()[:D])
    out = torch.empty_like(partial)
    n = 16 * D
    w_ok = (ctypes.c_float * n)(*[1.0] * n)
    w_neg = (ctypes.c_float * n)(*([1.0] * (n - 1) + [-0.5]))
    w_nan = (ctypes.c_float * n)(*([float('nan')] + [1.0] * (n - 1)))
    w_inf = (ctypes.c_float * (B * n))(*([1.0] * (B * n - 1) + [float('inf')]))
    uncond = G.uncond_for(C.RQT_TINY, cond)

    def call():
        if keep8 is not None:
            return L.rqamd_rqt_sample_masked(h, ptr(partial), ptr(keep8), active, ptr(cond), B, cb, 1.0, tk, tp, 2, 0, 0, ptr(out), None)
        return L.rqamd_rqt_sample(h, ptr(partial), ptr(cond), B, cb, 0, 0, 1.0, tk, tp, 2, 0, 0, ptr(out), None)

    def plain_again(ref):
        assert call() == 0                                 # (the refused call consumed the arming)
        sync()
        assert torch.equal(out, ref)
    sync()
    assert call() == 0
    sync()
    ref = out.clone()
    zp = ptr(z.contiguous())
    for w, pi in ((w_neg, 0), (w_nan, 0), (w_inf, 1)):
        assert L.rqamd_rqt_sample_anchor(h, zp, acb, acn, 64, w, pi) == 0
        assert call() == -1 and b'weight' in L.rqamd_last_error()
        plain_again(ref)
    nul = (ctypes.c_void_p * D)(*([acb[0]] * (D - 1) + [None]))
    for a, b in ((nul, acn), (acb, nul), (None, acn)):
        assert L.rqamd_rqt_sample_anchor(h, zp, a, b, 64, w_ok, 0) == 0
        assert call() == -1 and b'null codebook or norms' in L.rqamd_last_error()
        plain_again(ref)
    assert L.rqamd_rqt_sample_anchor(h, zp, acb, acn, 32, w_ok, 0) == 0
    assert call() == -2 and b'dim 32' in L.rqamd_last_error()
    plain_again(ref)
    assert L.rqamd_rqt_sample_anchor(h, zp, acb, acn, 64, w_ok, 0) == 0 and L.rqamd_rqt_sample_shared(h, 1) == 0
    assert call() == -2 and b'rqamd_rqt_sample_shared' in L.rqamd_last_error()
    plain_again(ref)
    ex = (ctypes.c_void_p * 1)(ptr(cond).value)
    wk = (ctypes.c_float * B)(*[0.5] * B)
    assert L.rqamd_rqt_sample_anchor(h, zp, acb, acn, 64, w_ok, 0) == 0 and L.rqamd_rqt_sample_compose(h, 1, ex, wk) == 0
    kp, pa = (None, None) if keep8 is None else (ptr(keep8), active)
    rc = L.rqamd_rqt_sample_guided(h, ptr(partial), kp, pa, ptr(cond), ptr(uncond), B, cb, 0, 0, 1.0, 2.0, tk, tp, 2, 0, 0, ptr(out), None)
    assert rc == -2 and b'rqamd_rqt_sample_compose' in L.rqamd_last_error()
    plain_again(ref)
    assert L.rqamd_rqt_sample_anchor(h, zp, acb, acn, 64, w_ok, 0) == 0 and L.rqamd_rqt_sample_anchor(h, None, None, None, 0, None, 0) == 0
    plain_again(ref)                                       # disarmed
    # and the entry point alone
    lg = torch.zeros((2, 500), dtype=torch.float32, device=partial.device)
    import pytest
    with pytest.raises(NotImplementedError, match='dim'):
        nat.anchor_logits(lg, torch.zeros((2, 32), device=partial.device), None, q.codebook_list(), q._norm_list(), torch.ones((2,), device=partial.device))
    with pytest.raises(ValueError, match='weight'):
        nat.anchor_logits(lg, z[:2, 0, 0], None, q.codebook_list(), q._norm_list(), torch.ones((3,), device=partial.device))
