"""Shared by tests/test_emu_sample_logp.py (host emulator) and tests/test_gpu_sample_logp.py (MI355X): the checks of the log-probabilities
of the draws -- rqamd_sample_logits_logp (the LOGP builds of the three sampler kernels), rqamd_rqt_sample_logp (the armed forms of the
four engine entry points) and RQTransformer.return_log_probs().  Matrices and parameter tables come from
tests/per_image_sampling_cases.py, the tiny models, conditionings and seeds from tests/masked_sampling_cases.py and
tests/guided_sampling_cases.py, guarded buffers from tests/sampler_check.py / tests/kernel_check.py.

Three kinds of comparison:
  exact      samples of a LOGP call against the call without log-probabilities; guided against unguided over guide_logits; +0.0 / NaN fills
  FILTERED   a filtered row's `draw` against log(float64(probs_out[r, code])) of the same kernel class: both sides are logf of the same
             fp32 number, two logf implementations of at most 2 ulp each -> 4 ulp = 2^-21 relative (of max(1, |draw|))
  measured   the streaming kernel's `draw` (no filter: its own online max / sum of exp) and the engine's `model` (the step form of
             log_prob_kernel) against fp64 log_softmax of the same fp32 logits.  A-priori: fp32 scaling x * (1 / T) (2 roundings, relative
             2^-23 of |x / T| <= ~12), expf (2 ulp per term), a sum of at most 16388 terms as 64 sequential adds + rescales per thread and a
             tree over 256 threads, logf: about 1e-5.  An observed value above 1e-4 is a bug in the reduction, not a tolerance.

Largest |error| observed per (vocabulary, class), emulator (host libm expf / logf) / MI355X:
    class    V       emulator    MI355X
    stream   16388   6.94e-07    8.56e-07
    stream   16384   6.84e-07    1.12e-06
    stream     500   3.80e-07    6.44e-07
    stream     499   4.63e-07    6.48e-07
    stream       7   1.39e-07    1.56e-07
    model      500   5.31e-07    9.79e-07      (the tiny engine, every form, graphs on and off, bf16 and fp16 engines)
(the unfiltered draws of the engine forms, V = 500: 5.33e-07 / 8.63e-07, under the stream bound).  Log-probabilities here are -2 .. -12,
where fp32 spacing is 2.4e-07 .. 9.5e-07: every figure is about one ulp of the result.  The bounds are 3 x the largest entry of the
class (the convention of tests/rqt_attn_cases.py): 3.36e-06 for the streaming kernel's draw, 2.94e-06 for model / model_uncond."""
import contextlib
import ctypes

import numpy as np
import torch

import guided_sampling_cases as G
import kernel_check as kc
import masked_sampling_cases as M
import per_image_sampling_cases as P
import sampler_check as S

VOCABS = P.VOCABS + (16388,)          # + the general kernel outside its register top-p path (V > 16384, V % 4 == 0)
FILTERED_REL = 2.0 ** -21             # 4 ulp: logf of the same fp32 probability on both sides
STREAM_MEASURED = 1.12e-06            # the largest entries of the table above
MODEL_MEASURED = 9.79e-07
STREAM_BOUND = 3 * STREAM_MEASURED
MODEL_BOUND = 3 * MODEL_MEASURED
A_PRIORI = 1e-4                       # above this a measured error is a bug in the reduction
ONEPASS_LOGP = 2 * 0.02               # one-pass against stepped logits: 0.02 per logit (tests/test_gpu_forward_onepass.py), twice that per log-probability
OBSERVED = {}

# scalar triples: two unfiltered ones over all 12 rows (the NaN row and the constant row in the streaming kernel), register kernel +
# hand-back, top-p alone (general kernel), top_k = 1
SCALARS = ((1.0, None, None), (0.7, None, None), (0.8, 10, 0.9), (1.0, None, 0.7), (1.0, 1, None))
ROW_SEEDS = [3, 2 ** 40 + 5, 3, 0, 7, 2 ** 62, 1, 9, 11, 13, 15, 17]
ROW_SCALES = [0.0, 1.0, 3.0, 1.5] * 3


def _note(key, value):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(value))
    return value


def filtered(V, k, p):
    return S.topk_on(k, V) or S.topp_on(p)


# ------------------------------------------------------------------------------------------------ the entry point, guarded
def call_logp(nat, logits, logits_u=None, scalar=None, rows=None, gscale=1.0, row_gscale=None, seeds=None, seed=11, offset=8, want_flags=True,
              expect=0):
    """rqamd_sample_logits_logp with caller-owned guarded outputs: scalar = (T, k or None, p or None), or rows = (T, K, P) device tensors
    (+ row_gscale, seeds).  The guards of samples_out, draw_logp_out and row_flags are checked here (nothing outside `rows` elements may
    be written).  -> (samples, draw, flags or None) as numpy, or None when the call is refused as expected"""
    R, V = logits.shape
    dev = logits.device
    sb, s = S.guarded_int((R,), torch.int64, dev)
    fb, f = S.guarded_int((R,), torch.int32, dev)
    db, d = kc.guarded((R,), torch.float32, dev)
    t, k, p = scalar if scalar is not None else (1.0, None, None)
    rt, rk, rp = rows if rows is not None else (None, None, None)
    with nat.on_device_of(logits):
        rc = nat.lib().rqamd_sample_logits_logp(nat.ptr(logits), nat.ptr(logits_u), R, V, float(t), 0 if k is None else int(k),
                                                -1.0 if p is None else float(p), float(gscale), nat.ptr(rt), nat.ptr(rk), nat.ptr(rp),
                                                nat.ptr(row_gscale), nat.ptr(seeds), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                                nat.ptr(s), nat.ptr(d), nat.ptr(f) if want_flags else None, nat.stream_of(logits))
    assert rc == expect, (rc, nat.lib().rqamd_last_error())
    if s.is_cuda:
        torch.cuda.synchronize(dev)
    S.check_guard_int(sb, R, 'samples_out')
    S.check_guard_int(fb, R, 'row_flags')
    kc.check_guard(db, R, 'draw_logp_out')
    if rc != 0:
        assert bool((s == S.SENTINEL).all()), 'samples_out was written by a refused call'
        kc.check_nan(d, 'draw_logp_out')
        return None
    if not want_flags:
        assert bool((f == S.SENTINEL).all()), 'row_flags was written'
    return s.cpu().numpy(), d.cpu().numpy(), f.cpu().numpy() if want_flags else None


def seeds_tensor(seeds, device):
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v for v in seeds], dtype=torch.int64, device=device)


_KERNEL_RUNS = {}


def kernel_runs(nat, V, device):
    """Every call of the kernel-level checks over the 12-row matrix of vocabulary V, made once per (device, V) and shared.
    'rows*': the per-row form over kernel_table(V); 'scalar': the triples of SCALARS.  Each entry: the LOGP call (samples, draw, flags), the
    samples of the entry point without log-probabilities, and the probs_out of that entry point's second call (same flags)."""
    key = (device.type, V)
    if key in _KERNEL_RUNS:
        return _KERNEL_RUNS[key]
    x = P.kernel_logits(V, V)
    logits = kc.poisoned(torch.from_numpy(x).to(device))
    table = P.kernel_table(V)
    T, K, Pp = P.table_tensors(table, device)
    sd = seeds_tensor(ROW_SEEDS, device)
    out = dict(x=x, table=table)
    for name, seeds, flags in (('rows', None, True), ('rows_seeds', sd, True), ('rows_noflags', None, False)):
        off = 0 if seeds is not None else 8
        got = call_logp(nat, logits, rows=(T, K, Pp), seeds=seeds, seed=11, offset=off, want_flags=flags)
        ref = S.call_rows(nat, logits, T, K, Pp, seeds, 11, off, want_probs=False, want_flags=flags)
        prob = S.call_rows(nat, logits, T, K, Pp, seeds, 11, off, want_probs=True, want_flags=flags)
        out[name] = (got, ref, prob)
    out['scalar'] = {}
    for (t, k, p), flags in [(trip, True) for trip in SCALARS] + [(SCALARS[2], False)]:      # (without row_flags: the general kernel alone)
        got = call_logp(nat, logits, scalar=(t, k, p), seed=11, offset=8, want_flags=flags)
        ref = S.call_scalar(nat, logits, t, k, p, 11, 8, want_probs=False, want_flags=flags)
        prob = S.call_scalar(nat, logits, t, k, p, 11, 8, want_probs=True, want_flags=flags) if filtered(V, k, p) else None
        out['scalar'][(t, k, p), flags] = (got, ref, prob)
    _KERNEL_RUNS[key] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. samples
def check_samples(nat, V, device):
    """the samples (and the hand-back flags) of a LOGP call are those of the call without log-probabilities, bit for bit: per-row form
    without seeds, with seeds, without row_flags; scalar form over SCALARS; and the binding's own wrapper once"""
    runs = kernel_runs(nat, V, device)
    for name in ('rows', 'rows_seeds', 'rows_noflags'):
        (s, d, f), ref, _ = runs[name]
        assert s.dtype == np.int64 and np.array_equal(s, ref.samples), (V, name, s, ref.samples)
        assert f is None or np.array_equal(f, ref.flags), (V, name)
        assert not np.isnan(d).any(), (V, name, d)
    for (trip, _), ((s, d, f), ref, _) in runs['scalar'].items():
        assert np.array_equal(s, ref.samples), (V, trip, s, ref.samples)
        assert f is None or np.array_equal(f, ref.flags), (V, trip)
    logits = torch.from_numpy(runs['x']).to(device)
    T, K, Pp = P.table_tensors(runs['table'], device)
    s, d = nat.sample_logits_logp(logits, row_temperature=T, row_top_k=K, row_top_p=Pp, seed=11, offset=8)
    assert np.array_equal(s.cpu().numpy(), runs['rows'][0][0]) and np.array_equal(d.cpu().numpy().view(np.uint32), runs['rows'][0][1].view(np.uint32))
    t, k, p = SCALARS[2]
    s, d = nat.sample_logits_logp(logits, temperature=t, top_k=k, top_p=p, seed=11, offset=8)
    assert np.array_equal(s.cpu().numpy(), runs['scalar'][SCALARS[2], True][0][0])
    assert np.array_equal(d.cpu().numpy().view(np.uint32), runs['scalar'][SCALARS[2], True][0][1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. filtered rows
def filtered_error(draw, prob_row, code, what=''):
    """|draw - log(float64(probs[code]))| against 2^-21 max(1, |draw|); returns the error in units of the bound"""
    q = float(prob_row[code])
    assert q > 0.0, f'{what}: the drawn code {code} has probability {q!r} in probs_out'
    want = float(np.log(np.float64(q)))
    err, bound = abs(float(draw) - want), FILTERED_REL * max(1.0, abs(float(draw)))
    assert err <= bound, f'{what}: draw {float(draw)!r} against log(probs_out) {want!r}: |err| {err:.3e} > {bound:.3e}'
    return err / bound


def check_filtered(nat, V, device):
    """rows with top-k and / or top-p in effect: `draw` is the log of the probability the kernel raced with -- that of probs_out of a
    second call, which changes neither the kernel class nor the samples of such rows.  top_k = 1 in effect: exactly +0.0."""
    runs = kernel_runs(nat, V, device)
    worst, n = 0.0, 0
    groups = [(name, [(r, runs['table'][r]) for r in range(12)], runs[name]) for name in ('rows', 'rows_seeds', 'rows_noflags')]
    groups += [(str(key), [(r, key[0]) for r in range(12)], run) for key, run in runs['scalar'].items()]
    for name, rows, ((s, d, _), ref, prob) in groups:
        for r, (t, k, p) in rows:
            if not filtered(V, k, p):
                continue
            assert int(prob.samples[r]) == int(s[r]), (V, name, r, 'probs_out changed the sample of a filtered row')
            worst = max(worst, filtered_error(d[r], prob.probs[r], int(s[r]), f'V {V} {name} row {r} {(t, k, p)}'))
            n += 1
            xr = runs['x'][r]
            if S.topk_on(k, V) and k == 1 and not np.isnan(xr).any() and int((xr == xr.max()).sum()) == 1:      # one survivor
                assert d[r].view(np.uint32) == 0, (V, name, r, 'top_k = 1 must give exactly +0.0', float(d[r]))
    assert n > 0
    print(f'V {V}: {n} filtered draws, largest |draw - log(probs_out)| = {worst:.3f} of the 2^-21 bound')
    _note(f'filtered/{V}', worst)


# ------------------------------------------------------------------------------------------------ 3. unfiltered rows
def logsoftmax64(x, T=1.0):
    """fp64 log_softmax(float64(x) / T) over the last axis, NaN treated as -inf"""
    with np.errstate(all='ignore'):
        z = np.asarray(x, np.float64) / float(np.float32(T))
        z = np.where(np.isnan(z), -np.inf, z)
        m = z.max(axis=-1, keepdims=True)
        return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def check_unfiltered(nat, V, device):
    """the streaming kernel: draw against fp64 log_softmax(x / T)[code], NaN as -inf -- every row of the matrix under the two unfiltered
    scalar triples (the NaN row; the constant row, where the result is -log V), and the unfiltered rows of the per-row calls"""
    runs = kernel_runs(nat, V, device)
    x = runs['x']
    worst = 0.0
    items = []
    for (trip, _), ((s, d, _), _, _) in runs['scalar'].items():
        if not filtered(V, trip[1], trip[2]):
            items += [(str(trip), r, trip[0], s, d) for r in range(12)]
    for name in ('rows', 'rows_seeds', 'rows_noflags'):
        (s, d, _), _, _ = runs[name]
        items += [(name, r, runs['table'][r][0], s, d) for r in range(12) if not filtered(V, *runs['table'][r][1:])]
    assert len(items) >= 24 + 12
    for name, r, t, s, d in items:
        want = logsoftmax64(x[r], t)[int(s[r])]
        assert np.isfinite(want), (V, name, r, 'a masked or NaN column was drawn')
        err = abs(float(d[r]) - want)
        worst = max(worst, err)
        if r == 11:
            assert abs(want + np.log(V)) < 1e-12                          # the constant row
    print(f'V {V}: {len(items)} unfiltered draws, largest |draw - fp64 log_softmax| = {worst:.3e} (bound {STREAM_BOUND:.3e})')
    _note(f'stream/{V}', worst)
    assert worst < A_PRIORI, f'V {V}: {worst:.3e} is beyond any rounding of the streaming reduction'
    assert worst <= STREAM_BOUND, f'V {V}: largest |draw - fp64 log_softmax| {worst:.3e} > {STREAM_BOUND:.3e}'
    return worst


# ------------------------------------------------------------------------------------------------ 4. guided rows
def check_guided(nat, V, device):
    """logits_u given: samples and draw equal, bit for bit, the unguided LOGP call over guide_logits(c, u, s) of the same rows -- per-row
    scales (0, 1, 3, 1.5 interleaved over kernel_table's classes), and scalar scales over one triple of each kernel"""
    c = torch.from_numpy(P.kernel_logits(V, V)).to(device)
    u = torch.from_numpy(P.kernel_logits(V, V + 1)).to(device)
    T, K, Pp = P.table_tensors(P.kernel_table(V), device)
    gs = torch.tensor(ROW_SCALES, dtype=torch.float32, device=device)
    g = torch.empty_like(c)
    for sc in sorted(set(ROW_SCALES)):
        idx = torch.tensor([i for i, v in enumerate(ROW_SCALES) if v == sc], device=device)
        g[idx] = nat.guide_logits(c[idx].contiguous(), u[idx].contiguous(), sc)
    assert np.array_equal(g[1::4].cpu().numpy().view(np.uint32), c[1::4].cpu().numpy().view(np.uint32))       # s = 1: the conditional rows
    for seeds in (None, seeds_tensor(ROW_SEEDS, device)):
        a = call_logp(nat, c, u, rows=(T, K, Pp), row_gscale=gs, seeds=seeds, offset=0 if seeds is not None else 8)
        b = call_logp(nat, g, rows=(T, K, Pp), seeds=seeds, offset=0 if seeds is not None else 8)
        assert np.array_equal(a[0], b[0]), (V, 'per-row guided samples', a[0], b[0])
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (V, 'per-row guided draw', a[1], b[1])
        assert np.array_equal(a[2], b[2])
    for sc, trip in ((3.0, SCALARS[2]), (1.0, SCALARS[0]), (0.0, SCALARS[3])):
        gg = nat.guide_logits(c, u, sc)
        a = call_logp(nat, c, u, scalar=trip, gscale=sc)
        b = call_logp(nat, gg, scalar=trip)
        assert np.array_equal(a[0], b[0]), (V, sc, trip, 'scalar guided samples')
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (V, sc, trip, 'scalar guided draw', a[1], b[1])
    # a scalar scale with per-row parameters: row_gscale NULL
    a = call_logp(nat, c, u, rows=(T, K, Pp), gscale=3.0)
    b = call_logp(nat, nat.guide_logits(c, u, 3.0), rows=(T, K, Pp))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. refusals (guards: every call above)
def check_refusals(nat, device):
    x = torch.zeros((2, 8), device=device)
    T, K, Pp = (torch.ones(2, device=device), torch.zeros(2, dtype=torch.int32, device=device), -torch.ones(2, device=device))
    assert call_logp(nat, x, rows=(T, None, Pp), expect=-1) is None
    assert call_logp(nat, x, rows=(None, K, Pp), expect=-1) is None
    assert call_logp(nat, x, row_gscale=T, rows=(T, K, Pp), expect=-1) is None              # a scale per row without logits_u
    L = nat.lib()
    one = nat.ptr(x)
    assert L.rqamd_sample_logits_logp(one, None, 2, 8, 1.0, 0, -1.0, 1.0, None, None, None, None, None, 0, 0, None, one, None, None) == -1
    assert L.rqamd_sample_logits_logp(one, None, 2, 8, 1.0, 0, -1.0, 1.0, None, None, None, None, None, 0, 0, one, None, None, None) == -1
    assert L.rqamd_sample_logits_logp(None, None, 2, 8, 1.0, 0, -1.0, 1.0, None, None, None, None, None, 0, 0, one, one, None, None) == -1
    assert b'null' in L.rqamd_last_error()
    assert L.rqamd_sample_logits_logp(one, None, 0, 8, 1.0, 0, -1.0, 1.0, None, None, None, None, None, 0, 0, one, one, None, None) == 0


# ================================================================================================ engine level
HW, D, V_TINY = 16, 4, 500
FORMS = ('plain', 'start_loc', 'masked', 'guided', 'guided_masked', 'per_image', 'per_image_seeds')


def engine_mask(B):
    """a mixed per-image mask with a fully kept position in the middle and at the end (masked_sampling_cases.replay_mask)"""
    return torch.from_numpy(M.replay_mask(B, 4, 4, D, 9))


def form_call(form, B, device, cond, uncond, few=False):
    """-> (guided, partial, keyword arguments, seeds or None, per-image tables T [B], tk / tp [B][D], gs [B] or None, keep (B,HW,D) bool, start)
    few: every form carries guided_sampling_cases.few_mask (the emulator: three positions run)"""
    kw = dict(cond=cond)
    guided = form in ('guided', 'guided_masked', 'per_image')
    partial = G.random_codes((B, 4, 4, D), V_TINY, 4, device)
    keep = torch.zeros((B, HW, D), dtype=torch.bool)
    start, seeds = 0, None
    T, tk, tp, gs = [1.0] * B, [[V_TINY] * D for _ in range(B)], [[1.0] * D for _ in range(B)], None
    if form == 'start_loc':
        kw.update(start_loc=(1, 2), top_k=50, top_p=0.9)
        start = 6
        keep[:, :start] = True
        tk, tp = [[50] * D for _ in range(B)], [[0.9] * D for _ in range(B)]
    if form == 'masked':
        kw.update(keep_mask=engine_mask(B).to(device), **G.SAMPLERS[2])
        keep = engine_mask(B).view(B, HW, D).clone()
        tk, tp = [list(G.SAMPLERS[2]['top_k']) for _ in range(B)], [list(G.SAMPLERS[2]['top_p']) for _ in range(B)]
    if form == 'guided':
        kw.update(uncond=uncond, guidance_scale=3.0, top_k=50, top_p=0.9)
        tk, tp, gs = [[50] * D for _ in range(B)], [[0.9] * D for _ in range(B)], [3.0] * B
    if form == 'guided_masked':
        kw.update(uncond=uncond, guidance_scale=3.0, keep_mask=engine_mask(B).to(device))
        keep = engine_mask(B).view(B, HW, D).clone()
        gs = [3.0] * B
    if form in ('per_image', 'per_image_seeds'):
        grp = P.group_tensors(B, V_TINY, device)
        kw.update(grp)
        T = grp['temperature'].tolist()
        tk, tp = [[int(k)] * D for k in grp['top_k'].tolist()], [[float(p)] * D for p in grp['top_p'].tolist()]
        if form == 'per_image':
            gs = [P.SCALES[i] for i in P.group_of(B)]
            kw.update(uncond=uncond, guidance_scale=torch.tensor(gs, dtype=torch.float32, device=device))
        else:
            seeds = [11, 2 ** 40 + 3, 5, 7, 9, 13][:B]
    if few:
        fm = G.few_mask(B)
        keep = keep | fm.view(B, HW, D)
        keep[:, :start] = True
        kw['keep_mask'] = keep.view(B, 4, 4, D).to(device)
        kw.pop('start_loc', None)
        kw['start_loc'] = (0, 0)
    return guided, partial, kw, seeds, (T, tk, tp, gs), keep, start


def run_form(ar, aux, form, cond, uncond, armed, amp=False, seed=5, few=False):
    guided, partial, kw, seeds, tables, keep, start = form_call(form, partial_B(cond), cond.device, cond, uncond, few)
    fn = ar.sample_guided if guided else ar.sample
    M.seed_all(seed)
    with (ar.seeds(seeds) if seeds is not None else contextlib.nullcontext()):
        with (ar.return_log_probs() if armed else contextlib.nullcontext()):
            return fn(partial, aux, amp=amp, **kw)


def partial_B(cond):
    return cond.shape[0]


def head_ran(keep, start, masked):
    """(HW,) bool: the positions whose head stack runs -- from start_loc on; with a mask, those where some row draws some depth"""
    if masked:
        return ~keep.all(dim=2).all(dim=0)
    return torch.arange(HW) >= start


def check_engine_form(nat, ar, aux, form, cond, uncond, amp=False, few=False):
    """items 6 - 8 for one form under the current ar.use_graph: codes of the armed call == the unarmed call's; fill values; model /
    model_uncond and draw re-derived from the engine's own stepped teacher-forced logits of the drawn codes"""
    B, dev = cond.shape[0], cond.device
    guided, partial, kw, seeds, (T, tk, tp, gs), keep, start = form_call(form, B, dev, cond, uncond, few)
    want = run_form(ar, aux, form, cond, uncond, False, amp, few=few)
    codes, lp = run_form(ar, aux, form, cond, uncond, True, amp, few=few)
    # 6. codes
    assert torch.equal(codes, want), (form, 'the armed call drew other codes')
    assert type(lp).__name__ == 'SampleLogProbs' and lp._fields == ('draw', 'model', 'model_uncond')
    assert (lp.model_uncond is not None) == guided
    for t in (lp.draw, lp.model) + ((lp.model_uncond,) if guided else ()):
        assert t.shape == codes.shape and t.dtype == torch.float32 and t.device == codes.device
    draw, model = lp.draw.cpu().view(B, HW, D), lp.model.cpu().view(B, HW, D)
    masked = 'keep_mask' in kw
    if masked or start:
        assert torch.equal(codes.cpu().view(B, HW, D)[keep], partial.cpu().view(B, HW, D)[keep])
    # 8. fill values
    ran = head_ran(keep, start, masked)
    assert bool(((draw.view(torch.int32) == 0) | ~keep).all()), (form, 'draw is not +0.0 at a code that was not drawn')
    assert bool((torch.isfinite(draw) & (draw <= 0))[~keep].all()), (form, 'draw of a drawn code is not a finite log-probability')
    models = [('model', model)] + ([('model_uncond', lp.model_uncond.cpu().view(B, HW, D))] if guided else [])
    for name, m in models:
        assert bool(torch.isnan(m)[:, ~ran].all()), (form, name, 'not NaN where no head ran')
        assert bool(torch.isfinite(m)[:, ran].all()), (form, name, 'not finite where the head ran')
    # 7. re-derivation from the engine's logits: stepped, over the same number of rows
    xs2 = torch.cat([codes, codes]) if guided else codes
    c2 = torch.cat([cond, uncond]) if guided else cond
    assert ar.forward_mode == 'stepped'
    logits = ar.teacher_forced_logits(xs2.contiguous(), aux, cond=c2.contiguous(), amp=amp)
    for d, v in enumerate(ar.vocab_size):
        logits[..., d, v:] = float('-inf')
    Vw = logits.shape[-1]
    logits = logits.view(-1, HW, D, Vw)
    ls = logsoftmax64(logits.cpu().numpy())
    cz = codes.cpu().view(B, HW, D).numpy()
    worst_m = 0.0
    for i, (name, m) in enumerate(models):
        ref = np.take_along_axis(ls[i * B:(i + 1) * B], cz[..., None], -1)[..., 0]
        err = np.abs(m.numpy().astype(np.float64) - ref)[:, ran.numpy()]
        worst_m = max(worst_m, float(err.max()))
    _note('model/500', worst_m)
    Tt = torch.tensor(T, dtype=torch.float32, device=dev)
    worst_f = worst_s = 0.0
    n_f = n_s = 0
    for pos in np.flatnonzero(ran.numpy()):
        for d in range(D):
            drawn = ~keep[:, pos, d]
            if not bool(drawn.any()):
                continue
            x = logits[:B, pos, d].contiguous()
            if guided:
                x = ar._guide_rows(x, logits[B:, pos, d].contiguous(), gs)
            kd, pd = [r[d] for r in tk], [r[d] for r in tp]
            Kt = torch.tensor([0 if k >= Vw else k for k in kd], dtype=torch.int32, device=dev)
            Pt = torch.tensor(pd, dtype=torch.float32, device=dev)
            probs = None
            xn = x.cpu().numpy()
            for b in np.flatnonzero(drawn.numpy()):
                if filtered(Vw, kd[b], pd[b]):
                    if probs is None:
                        probs = nat.sample_logits_rows(x, Tt, Kt, Pt, want_probs=True, want_samples=False)[1].cpu().numpy()
                    worst_f = max(worst_f, filtered_error(draw[b, pos, d].numpy(), probs[b], int(cz[b, pos, d]), f'{form} image {b} position {pos} depth {d}'))
                    n_f += 1
                else:
                    err = abs(float(draw[b, pos, d]) - logsoftmax64(xn[b], T[b])[int(cz[b, pos, d])])
                    worst_s = max(worst_s, err)
                    n_s += 1
    assert n_f + n_s == int((~keep[:, ran]).sum())
    _note('stream/engine', worst_s)
    print(f'{form} amp={amp} graph={ar.use_graph}: model |err| {worst_m:.3e} (bound {MODEL_BOUND:.3e}); {n_f} filtered draws {worst_f:.3f} of the '
          f'bound; {n_s} unfiltered draws |err| {worst_s:.3e} (bound {STREAM_BOUND:.3e})')
    assert worst_m < A_PRIORI and worst_s < A_PRIORI
    assert worst_m <= MODEL_BOUND, f'{form}: model against fp64 log_softmax of the engine logits: |err| {worst_m:.3e} > {MODEL_BOUND:.3e}'
    assert worst_s <= STREAM_BOUND, f'{form}: unfiltered draw against fp64 log_softmax: |err| {worst_s:.3e} > {STREAM_BOUND:.3e}'
    return codes, lp


def check_sum_against_log_probs(ar, aux, codes, lp, cond, amp=False):
    """an unmasked, unguided call: sum(model) against log_probs(codes).sum() -- the one-pass path, other GEMM tiles: 2 x 0.02 per code"""
    one = ar.log_probs(codes, aux, cond=cond, amp=amp)
    one = one[0] if isinstance(one, tuple) else one
    diff = (lp.model.double() - one.double()).abs()
    print(f'model against log_probs: largest difference per code {float(diff.max()):.3e}, sums {float(lp.model.double().sum()):.4f} / {float(one.double().sum()):.4f}')
    assert float(diff.max()) <= ONEPASS_LOGP
    assert abs(float(lp.model.double().sum()) - float(one.double().sum())) <= ONEPASS_LOGP * codes.numel()


# ------------------------------------------------------------------------------------------------ 10. ABI
def check_abi(nat, ar, aux, cond, uncond, amp=False):
    """model_logp_uncond_out with an unguided call is RQAMD_ERR_INVALID; an armed call that fails consumes the arming (the next call
    writes none of the three buffers); all NULL disarms.  Every call here keeps every code: nothing is launched."""
    eng, cbs = ar._eng(amp), ar._checked_codebooks(aux)
    B = cond.shape[0]
    partial = G.random_codes((B, 4, 4, D), V_TINY, 3, cond.device)
    keep8 = torch.ones(partial.shape, dtype=torch.uint8, device=cond.device)
    out = torch.empty_like(partial)
    L, h = eng._L, eng._h
    tk, tp = (ctypes.c_int * D)(*[50] * D), (ctypes.c_float * D)(*[1.0] * D)
    active = (ctypes.c_uint8 * HW)()
    cb = nat._ptr_array(cbs[:D])

    def bufs():
        return [torch.full(partial.shape, float('nan'), dtype=torch.float32, device=cond.device) for _ in range(3)]

    def masked(p=True):
        return L.rqamd_rqt_sample_masked(h, nat.ptr(partial) if p else None, nat.ptr(keep8), active, nat.ptr(cond), B, cb, 1.0, tk, tp, 1, 0, 0, nat.ptr(out), None)

    def guided():
        return L.rqamd_rqt_sample_guided(h, nat.ptr(partial), nat.ptr(keep8), active, nat.ptr(cond), nat.ptr(uncond), B, cb, 0, 0, 1.0, 2.0, tk, tp, 1, 0, 0,
                                         nat.ptr(out), None)

    def sync():
        if cond.is_cuda:
            torch.cuda.synchronize(cond.device)
    assert L.rqamd_rqt_sample_logp(None, None, None, None) == -1
    # an armed call: draw +0.0 at every kept code, model NaN (no head ran)
    a, b, c = bufs()
    assert L.rqamd_rqt_sample_logp(h, nat.ptr(a), nat.ptr(b), None) == 0
    assert masked() == 0
    sync()
    assert bool((a.view(torch.int32) == 0).all()) and bool(torch.isnan(b).all()) and torch.equal(out, partial)
    # the next call is unarmed
    a.fill_(float('nan'))
    assert masked() == 0
    sync()
    assert bool(torch.isnan(a).all())
    # uncond buffer with an unguided call
    assert L.rqamd_rqt_sample_logp(h, nat.ptr(a), nat.ptr(b), nat.ptr(c)) == 0
    assert masked() == -1 and b'unguided' in L.rqamd_last_error()
    assert masked() == 0
    sync()
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(c).all())
    # ... and with a guided call
    assert L.rqamd_rqt_sample_logp(h, nat.ptr(a), nat.ptr(b), nat.ptr(c)) == 0
    assert guided() == 0
    sync()
    assert bool((a.view(torch.int32) == 0).all()) and bool(torch.isnan(b).all()) and bool(torch.isnan(c).all())
    # armed, then a call refused for a bad argument: the arming is gone
    a.fill_(float('nan'))
    assert L.rqamd_rqt_sample_logp(h, nat.ptr(a), None, None) == 0
    assert masked(p=False) == -1
    assert masked() == 0
    sync()
    assert bool(torch.isnan(a).all()), 'a failed call left the handle armed'
    # all NULL disarms
    assert L.rqamd_rqt_sample_logp(h, nat.ptr(a), None, None) == 0
    assert L.rqamd_rqt_sample_logp(h, None, None, None) == 0
    assert masked() == 0
    sync()
    assert bool(torch.isnan(a).all())


def check_host_loops_refuse(ar, aux, cond, uncond):
    B = cond.shape[0]
    partial = G.random_codes((B, 4, 4, D), V_TINY, 3, cond.device)
    ones = torch.ones(partial.shape, dtype=torch.bool, device=cond.device)
    import pytest
    with ar.return_log_probs():
        for kw in (dict(cached=False), dict(cached=False, temperature=torch.ones(B, device=cond.device))):
            with pytest.raises(NotImplementedError, match='cached=False'):
                ar.sample(partial, aux, cond=cond, keep_mask=ones, **kw)
            with pytest.raises(NotImplementedError, match='cached=False'):
                ar.sample_guided(partial, aux, cond=cond, uncond=uncond, keep_mask=ones, **kw)
        ar.sampler = 'torch'
        try:
            with pytest.raises(NotImplementedError, match="sampler='torch'"):
                ar.sample(partial, aux, cond=cond, keep_mask=ones)
            with pytest.raises(NotImplementedError, match="sampler='torch'"):
                ar.sample_guided(partial, aux, cond=cond, uncond=uncond, keep_mask=ones)
        finally:
            ar.sampler = 'philox'
        codes, lp = ar.sample(partial, aux, cond=cond, keep_mask=ones)
        assert torch.equal(codes, partial) and bool((lp.draw.view(torch.int32) == 0).all()) and bool(torch.isnan(lp.model).all())
    assert torch.equal(ar.sample(partial, aux, cond=cond, keep_mask=ones), partial)      # outside the block: codes alone
