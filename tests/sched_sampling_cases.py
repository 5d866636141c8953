"""Shared by tests/test_emu_sched_sampling.py (host emulator) and tests/test_gpu_sched_sampling.py (MI355X): the checks of sampling
schedules over positions and depths -- rqamd_rqt_sample_schedule through RQTransformer.schedule() on the tiny fixture models
(RQT_TINY: 4 x 4 x 4, V 500, 3 images; RQT_TINY_TXT: 2 images).  Models, conditionings and masks come from
tests/masked_sampling_cases.py and tests/guided_sampling_cases.py.  Every comparison is exact: the yardstick of a scheduled draw is
the per-row stand-alone sampler on the same logits with the schedule's values at that (image, position, depth), and the unscheduled
calls of sample() / sample_guided().

`keep` (a (B,H,W,D) bool mask or None) rides along everywhere: the GPU file runs whole maps, the emulator -- minutes for a whole map --
the three positions guided_sampling_cases.few_mask leaves; the checks then look at the drawn codes only."""
import math

import numpy as np
import pytest
import torch

import guided_sampling_cases as G
import masked_sampling_cases as M

SEED, OFFSET = 20261, 4 * 977      # what sample() takes in place of the generator's state (fix_rng)
B, H, W, D, V = 3, 4, 4, 4, 500
HW = H * W
PARAMS = ('temperature', 'top_k', 'top_p', 'guidance_scale', 'min_p', 'typical_p')


def fix_rng(ar):
    ar._draw_rng = lambda device, n: (SEED, OFFSET)


def partial_for(keep, device, b=B):
    """zeros, or -- with a mask -- random codes where a code is kept"""
    if keep is None:
        return torch.zeros((b, H, W, D), dtype=torch.long, device=device)
    codes = G.random_codes((b, H, W, D), V, 3, 'cpu')
    return torch.where(keep[:b], codes, torch.zeros_like(codes)).to(device)


def call(ar, aux, cond, keep=None, uncond=None, **kw):
    """sample() -- sample_guided() with `uncond` -- over partial_for(keep)"""
    b, dev = cond.shape[0], cond.device
    km = {} if keep is None else dict(keep_mask=keep[:b].to(dev))
    if uncond is not None:
        return ar.sample_guided(partial_for(keep, dev, b), aux, cond=cond, uncond=uncond, **km, **kw)
    return ar.sample(partial_for(keep, dev, b), aux, cond=cond, **km, **kw)


def drawn_of(keep, b=B):
    return torch.ones((b, HW, D), dtype=torch.bool) if keep is None else ~keep[:b].reshape(b, HW, D)


# ------------------------------------------------------------------------------------------------ schedules
def constant(value, shape, b=B, dtype=torch.float32):
    """a schedule that holds `value` (a number, or D per-depth values) everywhere: shape 'hw' (numbers only), 'hwd' or 'bhwd'"""
    per_depth = torch.as_tensor(value, dtype=dtype).reshape(-1)
    if shape == 'hw':
        assert per_depth.numel() == 1
        return per_depth.reshape(1, 1).expand(H, W).clone()
    t = per_depth.expand(D).reshape(1, 1, 1, D).expand(b, H, W, D).clone()
    return t if shape == 'bhwd' else t[0]


def distinct_schedule(per_image, trunc, guided, depth_T=True, b=B):
    """Every (image, position, depth) -- every (position, depth) of the shared form -- has values of its own, and the three row
    classes of the sampler alternate with (image + position + depth) % 3, so that a per-image schedule has all three in every step:
      0  no filter at all                                   -> the streaming kernel
      1  top-k on (distinct k = 3 + i), top-p on at even i   -> the register kernel
      2  top-k off, top-p on (0.5 + 0.002 i)                  -> the general kernel
    trunc: min-p on where i % 3 == 1 and typical on where i % 4 == 2 in the classes 1 and 2, off elsewhere; guided: scales
    0.5 + 0.02 i on both sides of 1.  depth_T False: the temperature depends on (image, position) alone (what a per-image call
    can be given).  Shapes (B, H, W, D) or (H, W, D)."""
    nb = b if per_image else 1
    i = torch.arange(nb * HW * D).view(nb, HW, D)
    bb, pp, dd = torch.meshgrid(torch.arange(nb), torch.arange(HW), torch.arange(D), indexing='ij')
    cls = (bb + pp + dd) % 3
    f = i.to(torch.float32)
    out = dict(temperature=0.7 + 0.005 * (f if depth_T else (bb * HW + pp).to(torch.float32)),
               top_k=torch.where(cls == 1, 3 + i, torch.full_like(i, V)),
               top_p=torch.where(cls == 2, 0.5 + 0.002 * f, torch.where((cls == 1) & (i % 2 == 0), 0.6 + 0.001 * f, torch.ones_like(f))))
    if trunc:
        out['min_p'] = torch.where((cls != 0) & (i % 3 == 1), 0.01 + 0.0005 * f, torch.zeros_like(f))
        out['typical_p'] = torch.where((cls != 0) & (i % 4 == 2), 0.6 + 0.002 * f, torch.ones_like(f))
    if guided:
        out['guidance_scale'] = 0.5 + 0.02 * f
    on = out['top_k'][out['top_k'] < V]
    assert len(torch.unique(on)) == on.numel() and len(torch.unique(out['temperature'])) == (nb * HW * D if depth_T else nb * HW)
    return {k: (v.view(nb, H, W, D) if per_image else v.view(H, W, D)).clone() for k, v in out.items()}


def tables(sched, device, b=B):
    """the schedule as (b, HW, D) device tensors of the dtypes the stand-alone samplers take; parameters it does not hold: off values"""
    off = dict(temperature=1.0, top_k=V, top_p=1.0, guidance_scale=1.0, min_p=0.0, typical_p=1.0)
    out = {}
    for name in PARAMS:
        t = torch.as_tensor(sched[name]) if name in sched else torch.tensor(off[name])
        t = t.to(torch.int32 if name == 'top_k' else torch.float32)
        if t.dim() == 2:
            t = t[None, :, :, None]
        elif t.dim() == 3:
            t = t[None]
        out[name] = t.expand(b, H, W, D).reshape(b, HW, D).contiguous().to(device)
    return out


def masked_logits(ar, logits):
    for d, v in enumerate(ar.vocab_size):
        logits[..., d, v:] = float('-inf')
    return logits


def step_logits(ar, aux, X, cond, uncond=None, amp=False):
    """the stepped teacher-forced logits of X, LogitMask applied: (b, HW, D, V) -- and those of the unconditional twins, from the same
    2b-row pass, when uncond is given.  Bit-identical to the logits the sampling loop saw (same rows per launch, same kernels)."""
    b = X.shape[0]
    if uncond is None:
        L = masked_logits(ar, ar.teacher_forced_logits(X, aux, cond=cond, amp=amp))
        return L.view(b, HW, D, -1), None
    eng, cbs = ar._eng(amp), ar._checked_codebooks(aux)
    L = ar._on_side_stream(X.device, lambda: eng.logits(torch.cat([X, X]).contiguous(), torch.cat([cond, uncond]).contiguous(), cbs))
    L = masked_logits(ar, L)
    return L[:b].reshape(b, HW, D, -1), L[b:].reshape(b, HW, D, -1)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. every index, by replay
def replay(nat, ar, aux, cond, sched, X, draw, keep=None, uncond=None, amp=False, seeds=None):
    """For every (p, d) some row draws at: the per-row stand-alone sampler over the teacher-forced logits of X, with the schedule's
    values at (:, p, d), the call's seed and offset + p * D + d, returns X[:, p, d] -- sample_logits_trunc where a min-p / typical
    value is on in the step, else sample_logits_logp (and, unguided, sample_logits_rows: the same codes) -- and its log-probability
    is `draw`, bit for bit.  -> the row classes seen in one step, at most"""
    b, dev = X.shape[0], X.device
    t = tables(sched, dev, b)
    L, Lu = step_logits(ar, aux, X, cond, uncond, amp)
    drawn = drawn_of(keep, b).to(dev)
    Xv, dv = X.view(b, HW, D), None if draw is None else draw.view(b, HW, D)
    sd = None if seeds is None else torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64, device=dev)
    most = 0
    for p in range(HW):
        for d in range(D):
            m = drawn[:, p, d]
            if not bool(m.any()):
                continue
            x = L[:, p, d].contiguous()
            xu = None if Lu is None else Lu[:, p, d].contiguous()
            v = {n: t[n][:, p, d].contiguous() for n in PARAMS}
            gs = None if xu is None else v['guidance_scale']
            step = dict(seed=0 if seeds else SEED, offset=(0 if seeds else OFFSET) + p * D + d)
            on = bool((v['min_p'] > 0).any()) or bool(((v['typical_p'] >= 0) & (v['typical_p'] < 1)).any())
            if on:
                s, _, lg = nat.sample_logits_trunc(x, xu, row_temperature=v['temperature'], row_top_k=v['top_k'], row_top_p=v['top_p'],
                                                   row_min_p=v['min_p'], row_typical_p=v['typical_p'], row_gscale=gs, row_seeds=sd,
                                                   want_logp=True, **step)
            else:
                s, lg = nat.sample_logits_logp(x, xu, row_temperature=v['temperature'], row_top_k=v['top_k'], row_top_p=v['top_p'],
                                               row_gscale=gs, row_seeds=sd, **step)
                if xu is None:
                    s2, _ = nat.sample_logits_rows(x, v['temperature'], v['top_k'], v['top_p'], seeds=sd, **step)
                    assert torch.equal(s2, s)
            assert torch.equal(s[m], Xv[:, p, d][m]), ('replay', p, d, s.tolist(), Xv[:, p, d].tolist(), {n: v[n].tolist() for n in PARAMS})
            if dv is not None:
                assert same_bits(lg[m], dv[:, p, d][m]), ('draw log-probability', p, d, lg.tolist(), dv[:, p, d].tolist())
            k_on = (v['top_k'] > 0) & (v['top_k'] < V)
            p_on = (v['top_p'] >= 0) & (v['top_p'] < 1)
            t_on = (v['min_p'] > 0) | ((v['typical_p'] >= 0) & (v['typical_p'] < 1))
            cls = torch.where(k_on, 1, torch.where(p_on | t_on, 2, 0))[m]
            most = max(most, len(torch.unique(cls)))
    return most


def check_replay_every_index(nat, ar, aux, cond, per_image, trunc, keep=None, uncond=None, amp=False):
    """a schedule with values of its own at every index, armed log-probabilities: replayed step by step (replay)"""
    b = cond.shape[0]
    sched = distinct_schedule(per_image, trunc, uncond is not None, b=b)
    with ar.schedule(**sched), ar.return_log_probs():
        X, lp = call(ar, aux, cond, keep, uncond)
    kept = ~drawn_of(keep, b).view(b, H, W, D).to(X.device)
    assert torch.equal(X[kept], partial_for(keep, X.device, b)[kept]) and bool((lp.draw[kept] == 0).all())
    with ar.schedule(**sched):
        assert torch.equal(call(ar, aux, cond, keep, uncond), X), 'the armed call drew other codes'
    most = replay(nat, ar, aux, cond, sched, X, lp.draw, keep, uncond, amp)
    if per_image and keep is None:
        assert most == 3, 'no step had all three row classes'
    return X, sched


# ------------------------------------------------------------------------------------------------ 1. constant == per-image == scalar
CONST_T, CONST_K, CONST_P = 0.9, [50, 50, 500, 500], [0.9, 1.0, 0.9, 1.0]      # (guided_sampling_cases.SAMPLERS[2]: all three kernels)
CONST_MP, CONST_TY, CONST_GS = [0.05, 0.0, 0.3, 0.02], [0.9, 0.8, 1.0, 0.5], 3.0


def check_constant(ar, aux, cond, keep=None, uncond=None, seeds=None, trunc=False, amp=False, shapes=('hw', 'hwd', 'bhwd')):
    """schedules that hold one set of values everywhere, in each of the three shapes, == the per-image call == the scalar call"""
    b, dev = cond.shape[0], cond.device
    kw = dict(temperature=CONST_T, top_k=CONST_K, top_p=CONST_P, amp=amp)
    if uncond is not None:
        kw['guidance_scale'] = CONST_GS
    if trunc:
        kw.update(min_p=CONST_MP, typical_p=CONST_TY)
    ctx = (lambda: ar.seeds(seeds)) if seeds is not None else (lambda: ar.schedule())     # (an empty schedule is no schedule)
    with ctx():
        scalar = call(ar, aux, cond, keep, uncond, **kw)
        rows = dict(kw, temperature=torch.full((b,), CONST_T, device=dev), top_k=torch.tensor([CONST_K] * b, device=dev),
                    top_p=torch.tensor([CONST_P] * b, device=dev))
        if trunc:
            rows.update(min_p=torch.tensor([CONST_MP] * b, device=dev), typical_p=torch.tensor([CONST_TY] * b, device=dev))
        assert torch.equal(call(ar, aux, cond, keep, uncond, **rows), scalar), 'the per-image call differs from the scalar call'
        for shape in shapes:
            # 'hw' holds one value for every depth: temperature (and the scale) take that shape, the per-depth lists the other two
            deep = 'hwd' if shape == 'hw' else shape
            sched = dict(temperature=constant(CONST_T, shape, b), top_k=constant(CONST_K, deep, b, torch.int64), top_p=constant(CONST_P, deep, b))
            if uncond is not None:
                sched['guidance_scale'] = constant(CONST_GS, shape, b)
            if trunc:
                sched.update(min_p=constant(CONST_MP, deep, b), typical_p=constant(CONST_TY, deep, b))
            with ar.schedule(**sched):
                got = call(ar, aux, cond, keep, uncond, amp=amp)
            assert torch.equal(got, scalar), (f'constant {shape} schedule differs from the scalar call', sorted(sched))
            # a partial schedule: the other parameters from the call's own arguments, in each of their forms
            rest = {k: v for k, v in (rows if shape == 'bhwd' else kw).items() if k not in ('temperature', 'amp')}
            with ar.schedule(temperature=sched['temperature']):
                got = call(ar, aux, cond, keep, uncond, amp=amp, **rest)
            assert torch.equal(got, scalar), (f'temperature-only {shape} schedule differs from the scalar call', sorted(rest))
    return scalar


# ------------------------------------------------------------------------------------------------ 3. replay through masks
def check_position_by_per_image_call(ar, aux, cond, X, sched, positions, uncond=None):
    """keep all of X except position p: the per-image call with the schedule's values at p draws X[:, p] again"""
    b, dev = X.shape[0], X.device
    t = tables(sched, dev, b)
    for p in positions:
        keep = torch.ones((b, HW, D), dtype=torch.bool)
        keep[:, p] = False
        kw = dict(temperature=t['temperature'][:, p, 0].contiguous(), top_k=t['top_k'][:, p].to(torch.int64).contiguous(),
                  top_p=t['top_p'][:, p].contiguous(), keep_mask=keep.view(b, H, W, D).to(dev))
        assert bool((t['temperature'][:, p] == t['temperature'][:, p, :1]).all())
        if 'min_p' in sched:
            kw.update(min_p=t['min_p'][:, p].contiguous(), typical_p=t['typical_p'][:, p].contiguous())
        if uncond is not None:
            assert bool((t['guidance_scale'][:, p] == t['guidance_scale'][:, p, :1]).all())
            got = ar.sample_guided(X, aux, cond=cond, uncond=uncond, guidance_scale=t['guidance_scale'][:, p, 0].contiguous(), **kw)
        else:
            got = ar.sample(X, aux, cond=cond, **kw)
        assert torch.equal(got, X), f'position {p}: the per-image call with its values draws other codes'


# ------------------------------------------------------------------------------------------------ 6. effect
def check_greedy_from(ar, aux, cond, split, keep=None, amp=False):
    """top-k 1 from position `split` on: the argmax of the teacher-forced logits there (steps whose top-2 gap is 0 aside); before
    it, the unscheduled call's codes"""
    b, dev = cond.shape[0], cond.device
    k = torch.full((H, W), V, dtype=torch.int64)
    k.view(-1)[split:] = 1
    plain = call(ar, aux, cond, keep, amp=amp)
    with ar.schedule(top_k=k):
        got = call(ar, aux, cond, keep, amp=amp)
    drawn = drawn_of(keep, b).to(dev)
    gv, pv = got.view(b, HW, D), plain.view(b, HW, D)
    assert torch.equal(gv[:, :split], pv[:, :split]), 'positions before the schedule changes differ from the unscheduled call'
    L, _ = step_logits(ar, aux, got, cond, amp=amp)
    top2 = torch.topk(L, 2, dim=-1)
    sure = drawn & (top2.values[..., 0] > top2.values[..., 1])
    sure[:, :split] = False
    assert bool(sure.any()) and torch.equal(gv[sure], top2.indices[..., 0][sure]), 'a top-k 1 position did not draw the argmax'
    assert not torch.equal(gv[:, split:][drawn[:, split:]], pv[:, split:][drawn[:, split:]]), 'top-k 1 changed no draw'
    return got


def check_guidance_halves(nat, ar, aux, cond, uncond, split, keep=None):
    """scale 1 before position `split`, 3 from it on, greedy (top-k 1 as a number): every code is the argmax of guided_step_logits
    with the scale of its position, and the call differs from both constant calls"""
    b, dev = cond.shape[0], cond.device
    s = torch.ones((H, W))
    s.view(-1)[split:] = 3.0
    with ar.schedule(guidance_scale=s):
        got = call(ar, aux, cond, keep, uncond, top_k=1)
    drawn = drawn_of(keep, b).to(dev)
    gv = got.view(b, HW, D)
    for scale, lo, hi in ((1.0, 0, split), (3.0, split, HW)):
        g = G.guided_step_logits(nat, ar, aux, got, cond, uncond, scale).view(b, HW, D, -1)
        top2 = torch.topk(g, 2, dim=-1)
        sure = drawn & (top2.values[..., 0] > top2.values[..., 1])
        sure[:, :lo] = False
        sure[:, hi:] = False
        assert bool(sure.any()) and torch.equal(gv[sure], top2.indices[..., 0][sure]), f'scale {scale}: a code is not the guided argmax'
        const = call(ar, aux, cond, keep, uncond, top_k=1, guidance_scale=scale)
        assert not torch.equal(const, got), f'the scheduled call equals the constant call at scale {scale}'
    return got


# ------------------------------------------------------------------------------------------------ 7. refusals
def refusal_cases(b=B):
    """(name, schedule keywords, call keywords, guided, exception)"""
    T = torch.full((H, W), 0.9)

    def bad_T(v):
        t = T.clone()
        t[2, 1] = v
        return t
    return [('shape (W, H+1)', dict(temperature=torch.ones((H + 1, W))), {}, False, ValueError),
            ('shape (B+1, H, W, D)', dict(top_p=torch.full((b + 1, H, W, D), 0.9)), {}, False, ValueError),
            ('shape (H, W, D+1)', dict(top_k=torch.full((H, W, D + 1), 5)), {}, False, ValueError),
            ('shape (H*W,)', dict(temperature=torch.ones(HW)), {}, False, ValueError),
            ('top_k float', dict(top_k=torch.full((H, W), 5.0)), {}, False, ValueError),
            ('temperature twice', dict(temperature=T), dict(temperature=0.8), False, ValueError),
            ('top_k twice', dict(top_k=torch.full((H, W), 5)), dict(top_k=10), False, ValueError),
            ('min_p twice', dict(min_p=torch.full((H, W), 0.1)), dict(min_p=0.2), False, ValueError),
            ('guidance twice', dict(guidance_scale=torch.full((H, W), 2.0)), dict(guidance_scale=2.0), True, ValueError),
            ('temperature zero', dict(temperature=bad_T(0.0)), {}, False, ValueError),
            ('temperature negative', dict(temperature=bad_T(-1.0)), {}, False, ValueError),
            ('temperature nan', dict(temperature=bad_T(float('nan'))), {}, False, ValueError),
            ('temperature inf', dict(temperature=bad_T(float('inf'))), {}, False, ValueError),
            ('min_p above 1', dict(min_p=torch.full((H, W, D), 1.5)), {}, False, ValueError),
            ('typical_p nan', dict(typical_p=torch.full((H, W), float('nan'))), {}, False, ValueError),
            ('guidance in sample()', dict(guidance_scale=torch.full((H, W), 2.0)), {}, False, ValueError),
            ('guidance inf', dict(guidance_scale=torch.full((H, W), float('inf'))), {}, True, ValueError)]


def check_refusals(ar, aux, cond, uncond, keep=None):
    """each refusal raises before anything is drawn and leaves nothing armed: the next plain call is the earlier plain call"""
    kw = dict(temperature=CONST_T, top_k=CONST_K, top_p=CONST_P)
    plain = call(ar, aux, cond, keep, **kw)
    for name, sched, extra, guided, exc in refusal_cases(cond.shape[0]):
        with pytest.raises(exc):
            with ar.schedule(**sched):
                call(ar, aux, cond, keep, uncond if guided else None, **extra)
        assert ar._schedule is None
        assert torch.equal(call(ar, aux, cond, keep, **kw), plain), f'{name}: the plain call after the refusal differs'
    saved, ar.sampler = ar.sampler, 'torch'
    try:
        with pytest.raises(NotImplementedError):
            with ar.schedule(temperature=torch.full((H, W), 0.9)):
                call(ar, aux, cond, keep)
    finally:
        ar.sampler = saved
    assert torch.equal(call(ar, aux, cond, keep, **kw), plain)
    return plain


def check_c_refusals(nat, ar, aux, cond, keep):
    """rqamd_rqt_sample_schedule at the C ABI: values the armed call refuses (RQAMD_ERR_INVALID, raised as ValueError), the arming
    consumed by a refused and by a failing call, all NULL disarms, a wrong length refused by the binding"""
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    b, dev = cond.shape[0], cond.device
    partial = partial_for(keep, dev, b)
    k8 = keep[:b].to(torch.uint8).contiguous().to(dev)
    pa = [bool(a) for a in drawn_of(keep, b).any(dim=2).any(dim=0).tolist()]
    run = lambda T=CONST_T: eng.sample_masked(partial, k8, pa, cond, cbs, T, CONST_K, CONST_P, SEED, OFFSET, False)
    plain = run()
    n = HW * D
    assert eng._L.rqamd_rqt_sample_schedule(None, None, None, None, None, None, None, 0) == -1
    eng.arm_schedule(temperature=[0.5] * n)
    armed = run()
    assert not torch.equal(armed, plain) and torch.equal(run(), plain)                     # consumed by the call
    eng.arm_schedule(temperature=[0.5] * n)
    eng.arm_schedule()                                                                     # disarms
    assert torch.equal(run(), plain)
    for bad in (dict(temperature=[0.5] * (n - 1) + [0.0]), dict(temperature=[float('nan')] * n), dict(temperature=[float('inf')] * n),
                dict(min_p=[1.5] * n), dict(typical_p=[float('inf')] * n), dict(guidance_scale=[2.0] * n),
                dict(per_image=True, temperature=[0.5] * (b * n - 1) + [-1.0])):
        eng.arm_schedule(**bad)
        with pytest.raises(ValueError):
            run()
        assert torch.equal(run(), plain), bad                                              # consumed by the refused call
    eng.arm_schedule(temperature=[0.5] * n)
    with pytest.raises(ValueError):                                                        # refused before sample_impl: still consumed
        run(T=0.0)
    assert torch.equal(run(), plain)
    eng.arm_schedule(temperature=[0.5] * (n + 1))
    with pytest.raises(ValueError):
        run()
    assert torch.equal(run(), plain)
    # a per-image schedule in front of a scalar entry point: valid
    eng.arm_schedule(per_image=True, temperature=[0.5] * (b * n))
    assert torch.equal(run(), armed)


# ------------------------------------------------------------------------------------------------ 8. position_ramp
def check_position_ramp(ar):
    for kind in ('linear', 'cosine'):
        for start, end in ((1.0, 4.0), (1.2, 0.6), (2.0, 2.0)):
            r = ar.position_ramp(start, end, kind)
            assert tuple(r.shape) == (H, W) and r.dtype == torch.float32
            flat = r.reshape(-1)
            assert float(flat[0]) == np.float32(start) and float(flat[-1]) == np.float32(end)
            step = flat[1:] - flat[:-1]
            assert bool((step >= 0).all()) if end >= start else bool((step <= 0).all()), (kind, start, end)
            if end != start:
                assert len(torch.unique(flat)) > HW // 2
    lin = ar.position_ramp(0.0, 15.0).reshape(-1)
    assert torch.equal(lin, torch.arange(16, dtype=torch.float32))
    cos = ar.position_ramp(0.0, 1.0, 'cosine').reshape(-1)
    assert abs(float(cos[5]) - (1 - math.cos(math.pi * 5 / 15)) / 2) < 1e-6 and float(cos[1]) < float(lin[1]) / 15
    with pytest.raises(ValueError):
        ar.position_ramp(0.0, 1.0, 'step')
