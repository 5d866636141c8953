"""Shared by tests/test_emu_shared_cond.py (host emulator) and tests/test_gpu_shared_cond.py (MI355X): the end-to-end checks of shared-prompt
sampling -- rqamd_rqt_sample_shared, rqamd_rqt_kv_bytes and RQTransformer.shared_cond(n).

The contract is exactness against the plain call with every prompt repeated: with model.shared_cond(n), sample(partial, cond=cond_G) draws
image r as sample(partial, cond=cond_G.repeat_interleave(n, 0)) draws it.  Wherever the prefill over G prompts and the prefill over G * n
rows run the same GEMM tiles (both at most 128 rows here) the codes and log-probabilities are equal bit for bit; the one test across
regimes compares model log-probabilities within the project's path-to-path bound (ONEPASS_LOGP of tests/sample_logp_cases.py).

Two models with the same weights are used throughout, one for the shared calls and one for the plain ones: a handle's KV workspace has one
layout at a time, and a test that alternated the forms on one handle would re-lay it at every call."""
import numpy as np
import torch

from oracle import configs as C

import masked_sampling_cases as M
from sample_logp_cases import ONEPASS_LOGP

SAMPLER = dict(top_k=50, top_p=0.9)
SETUPS = {'tiny': ('RQT_TINY_TXT', 2, 4), 'txt32': ('RQT_TXT32', 2, 2), 'txt64': ('RQT_TXT64', 1, 2)}
FORMS = ('plain', 'keep_mask', 'start_loc', 'seeds', 'log_probs', 'truncation', 'schedule', 'guided+log_probs', 'one_pass+start_loc', 'amp')
# the forms composed, for the emulator (a sampling call of the tiny model takes it a minute): three calls that touch every form but amp
FORMS_COMPOSED = ('plain', 'keep_mask+seeds+log_probs+truncation+schedule', 'guided+log_probs+one_pass+start_loc')
_SETUPS = {}


class Setup:
    pass


def setup(name, device, seed=41):
    """models and inputs of one fixture, built once per (fixture, device) and never written to"""
    key = (name, str(device))
    if key in _SETUPS:
        return _SETUPS[key]
    s = Setup()
    cfg_name, s.G, s.fan = SETUPS[name]
    s.cfg = getattr(C, cfg_name)
    s.shared, s.aux = M.model(s.cfg, seed, device)
    s.plain, s.aux_p = M.model(s.cfg, seed, device)
    s.B = s.G * s.fan
    H, W, D = s.cfg['block_size']
    s.H, s.W, s.D = H, W, D
    s.cond = M.cond_for(s.cfg, s.G, device, seed=5)
    s.uncond = M.cond_for(s.cfg, s.G, device, seed=6)
    s.cond2 = M.cond_for(s.cfg, s.G, device, seed=7)
    rng = np.random.default_rng(seed + 1)
    s.partial = torch.from_numpy(rng.integers(0, min(s.shared.vocab_size), (s.B, H, W, D))).to(device)
    s.keep = torch.from_numpy(rng.random((s.B, H, W, D)) < 0.4).to(device)
    s.device = device
    _SETUPS[key] = s
    return s


# A guided call runs twice the rows through both prefills: 2 G P against 2 G n P.  With the shapes above that is 124 against 248 rows on
# RQT_TXT32 and 126 against 252 on RQT_TXT64 -- the plain call leaves the <= 128-row GEMM regime and exactness is no longer
# promised (measured on MI355X: codes differ).  The guided form therefore runs on the first (G, n) images of the same setup that keep both
# prefills at or below 128 rows: 62 against 124 on RQT_TXT32, 126 against 126 (n = 1) on RQT_TXT64.
GUIDED_SHAPE = {'tiny': (2, 4), 'txt32': (1, 2), 'txt64': (1, 1)}


def guided_setup(s, name):
    """the first G x n images of `s` (same models) for the guided form"""
    G, fan = GUIDED_SHAPE[name]
    if (G, fan) == (s.G, s.fan):
        return s
    if not hasattr(s, '_guided'):
        g = Setup()
        g.__dict__.update({k: v for k, v in s.__dict__.items() if not k.startswith('_')})
        g.G, g.fan, g.B = G, fan, G * fan
        g.partial, g.keep = s.partial[:g.B].contiguous(), s.keep[:g.B].contiguous()
        g.cond, g.uncond, g.cond2 = (c[:G].contiguous() for c in (s.cond, s.uncond, s.cond2))
        s._guided = g
    return s._guided


def forget():
    _SETUPS.clear()


def rep(s, c):
    return c.repeat_interleave(s.fan, 0).contiguous()


def same(a, b, what):
    """codes, or (codes, SampleLogProbs): equal bit for bit (NaN payloads and signed zeros included)"""
    if isinstance(a, tuple):
        assert torch.equal(a[0], b[0]), f'{what}: codes differ'
        for name in ('draw', 'model', 'model_uncond'):
            x, y = getattr(a[1], name), getattr(b[1], name)
            assert (x is None) == (y is None), (what, name)
            if x is not None:
                assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)), f'{what}: lp.{name} differs'
    else:
        assert torch.equal(a, b), f'{what}: codes differ ({int((a != b).sum())} of {a.numel()})'


def call(s, ar, form, cond, uncond, seed=11):
    """one sampling call on `ar` with the given conditioning rows (one per group inside shared_cond, one per image outside).  `form`: names
    joined by '+' -- plain, keep_mask, start_loc, late (start_loc = (3, 2): most positions run the body stack only), seeds, log_probs,
    truncation, schedule, guided, amp, one_pass (the caller's business: prefix_mode of the shared model)"""
    names = set(form.split('+'))
    assert names <= {'plain', 'keep_mask', 'start_loc', 'late', 'seeds', 'log_probs', 'truncation', 'schedule', 'guided', 'amp', 'one_pass'}, form
    kw = dict(SAMPLER)
    ctxs = []
    fn = ar.sample
    if 'keep_mask' in names:
        kw['keep_mask'] = s.keep
    if 'start_loc' in names or 'late' in names:
        kw['start_loc'] = (3, 2) if 'late' in names else (1, 2)
    if 'seeds' in names:
        ctxs.append(ar.seeds([100 + 3 * b for b in range(s.B)]))
    if 'log_probs' in names:
        ctxs.append(ar.return_log_probs())
    if 'truncation' in names:
        ctxs.append(ar.truncation(min_p=0.02, typical_p=0.95))
    if 'schedule' in names:
        ctxs.append(ar.schedule(temperature=ar.position_ramp(1.2, 0.8)))
    if 'guided' in names:
        fn = ar.sample_guided
        kw.update(uncond=uncond, guidance_scale=2.0)
    if 'amp' in names:
        kw['amp'] = True
    M.seed_all(seed)
    for c in ctxs:
        c.__enter__()
    try:
        return fn(s.partial, s.aux if ar is s.shared else s.aux_p, cond=cond, **kw)
    finally:
        for c in reversed(ctxs):
            c.__exit__(None, None, None)


def plain_result(s, form, which='cond'):
    """the plain repeated-cond call of `form` on the plain model (prefix_mode 'stepped'), computed once per (form, prompts) and shared"""
    memo = s.__dict__.setdefault('_plain', {})
    if (form, which) not in memo:
        s.plain.prefix_mode = 'stepped'
        memo[(form, which)] = call(s, s.plain, form, rep(s, getattr(s, which)), rep(s, s.uncond))
    return memo[(form, which)]


def codes_of(r):
    return r[0] if isinstance(r, tuple) else r


def check_form(s, form, graphs=(True, False)):
    """the shared call of `form`, with graphs and eager, against the plain repeated-cond call ('one_pass': the shared model runs with
    prefix_mode = 'one_pass' and is compared against the plain STEPPED call)"""
    want = plain_result(s, form)
    s.shared.prefix_mode = 'one_pass' if 'one_pass' in form.split('+') else 'stepped'
    try:
        for g in graphs:
            s.shared.use_graph = g
            with s.shared.shared_cond(s.fan):
                got = call(s, s.shared, form, s.cond, s.uncond)
            same(got, want, f'{form}, graphs {g}')
    finally:
        s.shared.use_graph = True
        s.shared.prefix_mode = 'stepped'
    codes = codes_of(want)
    assert int(codes.min()) >= 0 and int(codes.max()) < max(s.shared.vocab_size)
    if 'keep_mask' not in form and 'start_loc' not in form and 'late' not in form:
        assert not bool((codes == s.partial).all()), 'nothing was drawn'
    return want


def check_fan_one(s, form='plain'):
    """shared_cond(1): the shared path with one image per prompt equals the plain call"""
    want = plain_result(s, form)
    with s.shared.shared_cond(1):
        got = call(s, s.shared, form, rep(s, s.cond), None)
    same(got, want, 'shared_cond(1)')


def check_second_call_and_back(s, form='plain', graphs=True):
    """a second shared call with other prompts equals its own plain call (a stale group cache would show) and captures nothing; a plain
    call on the same model afterwards equals the plain call of a model that never ran a shared one, and the shared call after that the
    first one.  graphs: stream capture exists (not on the emulator, where every call runs eagerly and the counter stays 0)"""
    eng = s.shared._eng()
    with s.shared.shared_cond(s.fan):
        first = call(s, s.shared, form, s.cond, None)
        n = eng.graph_captures()
        assert n >= 1 if graphs else n == 0
        second = call(s, s.shared, form, s.cond2, None)
        assert eng.graph_captures() == n, 'the second shared call captured graphs'
    same(first, plain_result(s, form), 'first shared call')
    want2 = plain_result(s, form, 'cond2')
    same(second, want2, 'second shared call, other prompts')
    assert not torch.equal(first, second), 'the prompts made no difference'
    same(call(s, s.shared, form, rep(s, s.cond2), None), want2, 'a plain call after shared calls')
    with s.shared.shared_cond(s.fan):                                  # ... and shared again, on the re-laid workspace
        same(call(s, s.shared, form, s.cond, None), first, 'a shared call after a plain one')


def al(n):
    return (n + 255) & ~255


def check_memory(s):
    """rqamd_rqt_kv_bytes after a shared call: (batch H W + groups P) body slots per layer + the unchanged head caches, each allocation
    rounded up to 256 bytes -- below the plain call's (batch (H W + P) body slots)"""
    cfg = s.cfg
    E, HW, D, P = cfg['embed_dim'], s.H * s.W, s.D, cfg['block_size_cond'] - 1
    nb, nhd = cfg['body']['n_layer'], cfg['head']['n_layer']
    # models of their own (the workspaces of the shared ones have served other batches), and calls in which every code is kept: the
    # workspace is laid out and the prefix prefilled, no position runs
    keep = torch.ones((s.H, s.W), dtype=torch.bool, device=s.device)
    a, aux = M.model(cfg, 41, s.device)
    assert a._eng().kv_bytes() == 0
    with a.shared_cond(s.fan):
        assert torch.equal(a.sample(s.partial, aux, cond=s.cond, keep_mask=keep, **SAMPLER), s.partial)
    head = 2 * al(s.B * E * D * 2) * nhd
    want = 2 * al(s.B * E * HW * 2) * nb + 2 * al(s.G * E * P * 2) * nb + head
    got = a._eng().kv_bytes()
    assert got == want, (got, want)
    b, auxb = M.model(cfg, 41, s.device)
    b.sample(s.partial, auxb, cond=rep(s, s.cond), keep_mask=keep, **SAMPLER)
    plain = b._eng().kv_bytes()
    assert plain == 2 * al(s.B * E * (HW + P) * 2) * nb + head, plain
    assert got < plain
    a.sample(s.partial, aux, cond=rep(s, s.cond), keep_mask=keep, **SAMPLER)      # the other form on the same handle: laid out again
    assert a._eng().kv_bytes() == plain
    return got, plain


def check_errors(nat, device, monkeypatch, pytest, form='plain'):
    """every refusal, on the host before anything is enqueued; the arming is consumed by a failed call and the handle samples correctly
    afterwards"""
    s = setup('tiny', device)
    ar, aux = s.shared, s.aux
    want = plain_result(s, form)
    with pytest.raises(ValueError, match='n must be >= 1'):
        with ar.shared_cond(0):
            pass
    with ar.shared_cond(3):                                            # 8 images in groups of 3
        with pytest.raises(ValueError, match='not a multiple'):
            call(s, ar, 'plain', s.cond, None)
    with ar.shared_cond(s.fan):
        with pytest.raises(ValueError, match='one row per group'):
            call(s, ar, 'plain', rep(s, s.cond), None)                # cond with a row per image
        with pytest.raises(ValueError, match='one row per group'):
            call(s, ar, 'guided', s.cond, rep(s, s.uncond))
        with pytest.raises(NotImplementedError, match='shared_cond'):
            ar.sample(s.partial, aux, cond=s.cond, cached=False, **SAMPLER)
        ar.sampler = 'torch'
        try:
            with pytest.raises(NotImplementedError, match='shared_cond'):
                ar.sample(s.partial, aux, cond=s.cond, **SAMPLER)
        finally:
            ar.sampler = 'philox'
    # the library's own refusals, through the engine object: the arming is consumed by the failed call
    eng = ar._sampling_eng()
    cbs = ar._checked_codebooks(aux)
    args = (s.partial, None, cbs, (0, 0), 1.0, [50] * s.D, [0.9] * s.D, 1, 0, True)
    with pytest.raises(ValueError, match='fan = -2'):
        nat.check(eng._L.rqamd_rqt_sample_shared(eng._h, -2), eng._L)
    eng.arm_shared(0)                                                  # (the binding's own check of B % fan aside: the library's)
    assert eng._L.rqamd_rqt_sample_shared(eng._h, 3) == 0
    with pytest.raises(ValueError, match='not a multiple of the group size 3'):
        eng.sample(s.partial, rep(s, s.cond), *args[2:])
    same(call(s, ar, form, rep(s, s.cond), None), want, 'the call after a refused one is a plain call (arming consumed)')
    with ar.shared_cond(s.fan):
        same(call(s, ar, form, s.cond, None), want, 'a shared call after the refusals')
    # nothing to share: block_size_cond = 1
    ar1, aux1 = M.model(C.RQT_TINY, 41, device)
    p1 = torch.zeros((4, 4, 4, 4), dtype=torch.long, device=device)
    c1 = M.cond_for(C.RQT_TINY, 2, device)
    with ar1.shared_cond(2):
        with pytest.raises(NotImplementedError, match='no text prefix to share'):
            ar1.sample(p1, aux1, cond=c1, **SAMPLER)
    assert int(ar1.sample(p1, aux1, cond=c1.repeat_interleave(2, 0), start_loc=(3, 2), **SAMPLER).min()) >= 0
    # a body head size other than 64
    arh, auxh = M.model(C.RQT_TINY_TXT_HEADS, 41, device)
    with arh.shared_cond(s.fan):
        with pytest.raises(NotImplementedError, match='head size'):
            arh.sample(s.partial, auxh, cond=s.cond, **SAMPLER)
    # the 8-bit cache formats
    for fmt in ('int8k', 'int8kv'):
        monkeypatch.setenv('RQAMD_KV', fmt)
        ar8, aux8 = M.model(s.cfg, 41, device)
        with ar8.shared_cond(s.fan):
            with pytest.raises(NotImplementedError, match='RQAMD_KV=' + fmt):
                ar8.sample(s.partial, aux8, cond=s.cond, **SAMPLER)
        monkeypatch.delenv('RQAMD_KV')
    # a body context over 256
    import copy
    big = copy.deepcopy(C.RQT_TINY_TXT)
    big['block_size_cond'], big['vocab_size_cond'] = 250, 20
    arb, auxb = M.model(big, 41, device)
    with arb.shared_cond(s.fan):
        with pytest.raises(NotImplementedError, match='body context 265 > 256'):
            arb.sample(s.partial, auxb, cond=M.cond_for(big, s.G, device), **SAMPLER)


def check_guided_across_regimes(s):
    """the guided call at the full (G, n) of a wide setup (RQT_TXT32 2 x 2, RQT_TXT64 1 x 2), where GUIDED_SHAPE steps down because the plain
    call's doubled prefill leaves the 128-row regime: the same comparison as check_across_regimes.  keep_mask keeps depths 0 .. D-2 of
    position 0, whose model log-probabilities (conditional and unconditional) depend on the prefix and on given codes only: within
    ONEPASS_LOGP, the project's path-to-path bound.  Groups of n >= 2 rows share both the conditional and the unconditional prefix here"""
    assert s.fan >= 2
    keep = torch.zeros((s.H, s.W, s.D), dtype=torch.bool, device=s.device)
    keep[0, 0, :s.D - 1] = True
    kw = dict(SAMPLER, keep_mask=keep, guidance_scale=2.0)
    out = {}
    for name in ('shared', 'plain'):
        M.seed_all(5)
        if name == 'shared':
            with s.shared.return_log_probs(), s.shared.shared_cond(s.fan):
                out[name] = s.shared.sample_guided(s.partial, s.aux, cond=s.cond, uncond=s.uncond, **kw)
        else:
            with s.plain.return_log_probs():
                out[name] = s.plain.sample_guided(s.partial, s.aux_p, cond=rep(s, s.cond), uncond=rep(s, s.uncond), **kw)
    assert torch.equal(out['shared'][0][:, 0, 0, :s.D - 1], s.partial[:, 0, 0, :s.D - 1]), 'kept codes changed'
    worst = 0.0
    for field in ('model', 'model_uncond'):
        a, b = (getattr(out[n][1], field) for n in ('shared', 'plain'))
        assert a is not None and b is not None, field
        a, b = a[:, 0, 0, :s.D - 1].cpu(), b[:, 0, 0, :s.D - 1].cpu()
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), field
        err = float((a - b).abs().max())
        print('guided shared vs plain, %d x %d: lp.%s of the kept codes differs by at most %.5f' % (s.G, s.fan, field, err))
        assert err < ONEPASS_LOGP, (field, err)
        worst = max(worst, err)
    return worst


def check_across_regimes(device):
    """RQT_TXT64, 3 prompts x 43 images: the prefill runs over 189 rows in the shared call and over 8127 in the plain one -- other GEMM
    tiles.  keep_mask keeps depths 0 .. D-2 of position 0, so the model log-probabilities of those codes are those of the same codes under
    both prefills: within ONEPASS_LOGP, the project's path-to-path bound"""
    cfg, G, fan = C.RQT_TXT64, 3, 43
    B = G * fan
    H, W, D = cfg['block_size']
    ar, aux = M.model(cfg, 41, device)
    cond = M.cond_for(cfg, G, device)
    rng = np.random.default_rng(9)
    partial = torch.from_numpy(rng.integers(0, cfg['vocab_size'], (B, H, W, D))).to(device)
    keep = torch.zeros((H, W, D), dtype=torch.bool, device=device)
    keep[0, 0, :D - 1] = True
    out = {}
    for name in ('shared', 'plain'):
        M.seed_all(5)
        with ar.return_log_probs():
            if name == 'shared':
                with ar.shared_cond(fan):
                    out[name] = ar.sample(partial, aux, cond=cond, keep_mask=keep, **SAMPLER)
            else:
                out[name] = ar.sample(partial, aux, cond=cond.repeat_interleave(fan, 0), keep_mask=keep, **SAMPLER)
    a, b = (out[n][1].model[:, 0, 0, :D - 1].cpu() for n in ('shared', 'plain'))
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    err = float((a - b).abs().max())
    agree = float((out['shared'][0] == out['plain'][0]).float().mean())
    print('shared vs plain across GEMM regimes: model log-probabilities of the kept codes differ by at most %.5f; %.1f %% of all codes equal'
          % (err, 100 * agree))
    assert err < ONEPASS_LOGP, err
    return err
