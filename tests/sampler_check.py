"""Certificate checks of the on-device sampler (csrc/rqt_kernels.hip: sample_gumbel_kernel, sample_topk_kernel + sample_tail, sample_kernel,
each in its scalar, guided and per-row build) against an exact Philox reference and fp64 filters.  Shared by tests/test_gpu_sampler.py
(the MI355X), tests/test_emu_sampler.py (the host emulator) and tests/test_sampler_check.py (the evidence that these checks can fail).
Everything here is numpy in fp64 on the CPU; the GPU is only touched through the `nat` binding the runners are handed.

Stream.  Philox4x32-10 with counter (index / 4, row field, offset lo, offset hi), key (seed lo, seed hi), word index % 4, and
u = ((r >> 9) * 2 + 1) / 2^24: 23 random bits + a half, exact in fp32, so the reference's u IS the kernel's u.

Scaled logits.  x' = fl32(x / T) by a numpy float32 division (the filtered kernels divide), NaN -> -inf after top-k.

 1. top-k (exact): the live set is {i : not (x'_i < kth)} minus NaN / -inf columns, kth the k-th largest with NaN ranked first
    (torch.topk).  Ties at the threshold are all kept, a NaN threshold drops nothing, -0.0 == +0.0.
 2. probabilities (elementwise, c = 1 derived, not measured):
        |p - p64| <= c u (n0 + a_i) p64 + 2^-126,      u = 2^-24,  a_i = |x'_i - max x'|,
    p64 the fp64 softmax of x' over the certified kept set.  Roundings behind p_i = fl(e_i / z): the subtraction x'_i - max (relative
    u of a_i, which the exponential turns into a relative u a_i of e_i -- the a_i term), expf (1 ulp = 2 u), the division (u), and z:
    a sum of terms that each carry (2 + a_k) u, i.e. (2 + A) u with A = sum_k p64_k a_k, plus the depth of the fp32 summation
    d = max(ceil(V / 256), 8) + 10 (sequential adds of one thread -- the register kernel adds its 8 or 64 values in 4 chains, the
    general kernel ceil(V / 256) values in one --, 6 shuffle steps, 4 wavefront partials).  One division: n0 = d + 5 + A.  With top-p
    the row is divided twice: p_i = fl(q_i / kept), q_i = fl(e_i / z); z cancels, q_i carries (2 + a_i + 1) u, `kept` (3 + A) u over
    the kept set plus d u, and the second division u: n0 = d + 7 + A.  Dropped entries are exactly 0.0; rows sum to 1 within the sum
    of the elementwise bounds.
 3. top-p certificate.  With p64 the fp64 softmax over the live set of 1., E = u (n0 + A + d) (the bound of the kernel's fp32 mass
    of a set of its own probabilities: n0 + a_i per term, weighted mean <= A over a set of the largest terms, + d for the sum) and
    p = fl32(top_p), a kept set K is legitimate iff
      (i)   no dropped live entry has p64 above a kept one's by more than the two elementwise bounds of 2.;
      (ii)  among the live entries whose x' equals the smallest kept x', the kept ones are the lowest indices;
      (iii) mass64(K) >= p (1 - E), and K is a single token or mass64(K) - (its smallest member) < p (1 + E).
    top_p < 0 or >= 1 keeps everything.
 4. draw certificate, filtered kernels: teacher-forced on the kernel's own kept set K (probs_out > 0 of the same call), with p64 the
    fp64 softmax over K and s_i = p64_i / -log(u_i): the drawn j lies in K and s_j >= max_i s_i (1 - C_RACE u).
 5. draw certificate, streaming kernel (no filter, no probs_out): g_i = x_i / T - log(-log u_i) in fp64, NaN -> -inf; the drawn j has
    g_j >= max g - C_GUMBEL u max(1, |max g|); a -inf or NaN column is never drawn.
 6. certificate power (conditions on the inputs, checked on the CPU from the reference alone): the runner-up lies inside the tolerance
    of 4. / 5. in fewer than 1 % of rows; on tie-free rows exactly one sorted prefix satisfies 3.(iii) in at least 95 % of rows.
 7. memory: logits are the front views of NaN-filled buffers (kernel_check.poisoned), probs_out a view into a NaN-guarded buffer
    (kernel_check.guarded), samples_out and row_flags views into sentinel-guarded integer buffers (guarded_int).
 8. hand-back: where the register kernel runs (0 < k < V, V <= 16384, V % 4 == 0, row_flags given) it sets row_flags[r] = 1 iff the
    threshold is NaN or more than SMP_CAP keys are >= it, else 0; elsewhere row_flags is not written."""
import collections
import math

import numpy as np
import torch

import kernel_check as kc

U = 2.0 ** -24                 # fp32 unit roundoff
TINY = 2.0 ** -126             # smallest normal fp32
SMP_T, SMP_VPT, SMP_CAP, SMP_UND, V_MAX = 256, 64, 2048, 256, 36000      # csrc/rqt_kernels.hip
SENTINEL = -7                  # fill of integer outputs and their guards
M32 = np.uint64(0xFFFFFFFF)

# ------------------------------------------------------------------------------------------------ measured constants
# Both are measured against the REFERENCE arithmetic on the CPU, never against the kernel (measure() below; tests/test_sampler_check.py
# re-measures and compares).  RACE_MEASURED: over the rows of measure_inputs(), the largest error of a numpy-float32 model's race
# score (exp, sum, divide, [top-p: divide by the kept sum,] log, divide) of the two leading columns against their fp64 score, in units
# of u of the best score.  The top-p path adds one division per entry (1 u on either column; the kept sum is common to both): the
# model is run with it.  GUMBEL_MEASURED: the same for the float32 Gumbel score x * fl(1 / T) - log(-log u), in units of
# u max(1, |max g|).  A draw decided by scores that are each within d of the fp64 ones falls short of the best by at most 2 d:
# C = 4 x the measurement.
RACE_MEASURED = 10.6
GUMBEL_MEASURED = 1.93
C_RACE = 4.0 * RACE_MEASURED
C_GUMBEL = 4.0 * GUMBEL_MEASURED
# Observed on MI355X over every case of tests/test_gpu_sampler.py (printed under -s, recorded in profiles/sampler_certificate.txt; for
# information, no bound is derived from these): race deficit 0 u and Gumbel deficit 0 u -- every certified draw,
# the streaming kernel's native __logf included, is the argmax of the fp64 scores, so C_GUMBEL stays at its reference-side value --,
# probability ratio 0.502 of the derived bound (c = 1), top-p mass slack 0.056 E.

OBSERVED = {}


def _note(key, value):
    if value == value:
        OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(value))
    return value


# ------------------------------------------------------------------------------------------------ Philox
def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 over broadcastable integer arrays (uint64 arithmetic on 32-bit values) -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3, k0, k1 = [np.array(a, dtype=np.uint64) & M32 for a in np.broadcast_arrays(c0, c1, c2, c3, k0, k1)]
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def _u64(v, n):
    """python ints (any size below 2^64) or an array -> (n,) uint64"""
    if np.isscalar(v) or isinstance(v, int):
        return np.full((n,), int(v) & (2 ** 64 - 1), dtype=np.uint64)
    return np.array([int(s) & (2 ** 64 - 1) for s in v], dtype=np.uint64)


def words(V, rowfield, seed, offset, rounds=10):
    """the sampler's 32-bit word of every (row, vocabulary index): counter (i / 4, rowfield[r], offset lo, offset hi), key seed[r] lo /
    hi, word i % 4.  rowfield (R,), seed an int or (R,), offset an int -> (R, V) uint64"""
    R = len(rowfield)
    seed, off = _u64(seed, R)[:, None], np.uint64(int(offset) & (2 ** 64 - 1))
    i4 = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    out = philox4x32(i4, _u64(rowfield, R)[:, None], off & M32, off >> np.uint64(32), seed & M32, seed >> np.uint64(32), rounds)
    return np.stack(out, axis=-1).reshape(R, -1)[:, :V]


def u01(w):
    """rq_u01: ((w >> 9) * 2 + 1) / 2^24 in (0, 1), exact in fp32 and in fp64"""
    return ((w >> np.uint64(9)) * np.uint64(2) + np.uint64(1)).astype(np.float64) * U


# ------------------------------------------------------------------------------------------------ reference filters
def scaled(x, T):
    """x' = fl32(x / T): the division of the filtered kernels in numpy float32"""
    with np.errstate(all='ignore'):
        return (np.asarray(x, np.float32) / np.float32(T)).astype(np.float32)


def topk_on(k, V):
    return k is not None and 0 < k < V


def topp_on(p):
    return p is not None and 0.0 <= p < 1.0


def kth_largest(xs, k):
    """k-th largest of a float32 row, NaN ranked first (np.sort puts NaN last)"""
    return np.sort(xs)[::-1][k - 1]


def live_set(xs, k):
    """1.: boolean (V,) of the columns that survive top-k with a finite scaled logit, and the row's expected hand-back flag"""
    V = xs.shape[0]
    keep, flag = np.ones(V, bool), 0
    if topk_on(k, V):
        kth = kth_largest(xs, k)
        with np.errstate(invalid='ignore'):
            keep = ~(xs < kth)                         # NaN threshold: nothing is below it; NaN entries are not below anything
        flag = int(np.isnan(kth) or int(keep.sum()) > SMP_CAP)
    with np.errstate(invalid='ignore'):
        return keep & (xs > -np.inf), flag             # (NaN > -inf is False)


def softmax64(xs, K):
    """fp64 softmax of the float32 row xs over the boolean set K (zeros elsewhere) and a_i = |x'_i - max| (0 outside K)"""
    z = np.where(K, xs.astype(np.float64), -np.inf)
    m = z.max()
    with np.errstate(invalid='ignore'):
        a = np.where(K, m - z, 0.0)
    e = np.where(K, np.exp(-a), 0.0)
    return e / e.sum(), a


def sum_depth(V):
    return max(-(-V // SMP_T), 8) + 10


def prob_bound(p64, a, V, two_div):
    """2.: the elementwise bound at c = 1, and (n0, A)"""
    A = float((p64 * a).sum())
    n0 = sum_depth(V) + (7 if two_div else 5) + A
    return U * (n0 + a) * p64 + TINY, n0, A


def check_probs(p, p64, a, K, V, two_div, what=''):
    """2.: elementwise bound, exact zeros outside K, the row sum; returns the observed max (|p - p64| - 2^-126) / (u (n0 + a) p64)"""
    bound, n0, _ = prob_bound(p64, a, V, two_div)
    p = p.astype(np.float64)
    assert not np.isnan(p).any(), f'{what}: NaN probabilities'
    out = ~K & (p != 0.0)
    assert not out.any(), f'{what}: {int(out.sum())} nonzero probabilities outside the kept set (first at {int(np.flatnonzero(out)[0])})'
    err = np.abs(p - p64)
    bad = err > bound
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {V} probabilities outside the bound; first at {i}: {p[i]!r} against {p64[i]!r}, '
                             f'|err| {err[i]:.3e} > {bound[i]:.3e}')
    assert abs(p.sum() - 1.0) <= bound.sum(), f'{what}: the row sums to {p.sum()!r}'
    return _note('probability ratio', float(((err - TINY).clip(min=0.0)[K] / np.maximum(bound[K] - TINY, 1e-300)).max()))


def check_topp(kept, xs, L, V, top_p, what=''):
    """3.: is the kept set (boolean) legitimate for the float32 row xs with live set L?  Returns the mass slack used, in units of E"""
    p64, a = softmax64(xs, L)
    bound, n0, A = prob_bound(p64, a, V, False)
    E, p = U * (n0 + A + sum_depth(V)), float(np.float32(top_p))
    assert kept.any(), f'{what}: top-p kept nothing'
    assert not (kept & ~L).any(), f'{what}: top-p kept a column outside the top-k set'
    dropped = L & ~kept
    lo = int(np.flatnonzero(kept)[np.argmin(p64[kept])])                 # a smallest kept member
    if dropped.any():
        hi = int(np.flatnonzero(dropped)[np.argmax(p64[dropped])])
        assert p64[hi] - p64[lo] <= bound[hi] + bound[lo], f'{what}: dropped column {hi} (p {p64[hi]!r}) outranks kept column {lo} (p {p64[lo]!r})'
    tie = np.flatnonzero(L & (xs == xs[kept].min()))                        # (-0.0 == +0.0: equal logits, equal probabilities)
    nk = int(kept[tie].sum())
    assert kept[tie[:nk]].all(), f'{what}: the kept boundary ties {tie[kept[tie]].tolist()[:8]} are not the lowest indices of {tie.tolist()[:8]}'
    mass = float(p64[kept].sum())
    assert mass >= p * (1.0 - E), f'{what}: kept mass {mass!r} < top_p {p!r} (1 - {E:.3g}): the crossing token is missing'
    single = int(kept.sum()) == 1
    assert single or mass - p64[lo] < p * (1.0 + E), f'{what}: kept mass without column {lo} is {mass - p64[lo]!r} >= top_p {p!r} (1 + {E:.3g}): one token too many'
    used = max(p - mass, 0.0 if single else mass - p64[lo] - p, 0.0) / (p * E) if p > 0 else 0.0
    return _note('top-p mass slack / E', used)


def prefix_count(xs, L, V, top_p):
    """6.: how many sorted prefixes of the row satisfy 3.(iii) (one: the certificate pins the kept set)"""
    p64, a = softmax64(xs, L)
    _, n0, A = prob_bound(p64, a, V, False)
    E, p = U * (n0 + A + sum_depth(V)), float(np.float32(top_p))
    cum = np.cumsum(np.sort(p64[L])[::-1])
    before = np.concatenate([[0.0], cum[:-1]])
    ok = (cum >= p * (1.0 - E)) & ((before < p * (1.0 + E)) | (np.arange(len(cum)) == 0))
    return int(ok.sum())


# ------------------------------------------------------------------------------------------------ draw certificates
def race_deficit(p64, u, j):
    """4.: (relative deficit of column j's score against the best, in units of u; the same for the runner-up of the fp64 race)"""
    with np.errstate(divide='ignore'):
        s = p64 / -np.log(u)
    top = np.partition(s, -2)[-2:] if len(s) > 1 else np.array([0.0, s[0]])
    return (top[1] - s[j]) / top[1] / U, (top[1] - top[0]) / top[1] / U


def gumbel_scores(x, T, u):
    with np.errstate(all='ignore'):
        g = np.asarray(x, np.float64) / float(np.float32(T)) - np.log(-np.log(u))
    return np.where(np.isnan(g), -np.inf, g)


def gumbel_deficit(g, j):
    top = np.partition(g, -2)[-2:] if len(g) > 1 else np.array([-np.inf, g[0]])
    unit = U * max(1.0, abs(top[1]))
    return (top[1] - g[j]) / unit, (top[1] - top[0]) / unit


# ------------------------------------------------------------------------------------------------ the certifier
def certify(x, T, k, p, probs, samples, rowfield, seed, offset, what='', flags=None, register=False):
    """Everything of 1. - 5. and 8. for the rows of one call that share (T, k, p).  x (R, V) float32; probs (R, V) float32 or None;
    samples (R,) int64 or None; rowfield (R,), seed an int or (R,), offset an int: the stream of the rows; flags (R,) with `register`
    True where the register kernel must have run, False where it must not have written.  probs None and no filter in effect: the
    streaming kernel's certificate; probs None with top-k alone: the race on the exact top-k set; probs None with top-p: not
    certifiable (compare the samples with a call that has probs).
    Returns (largest deficit in units of u, number of rows whose runner-up lies inside the tolerance)."""
    x = np.asarray(x, np.float32)
    R, V = x.shape
    xs = scaled(x, T)
    filtered = topk_on(k, V) or topp_on(p)
    if samples is not None:
        assert samples.shape == (R,) and bool(((samples >= 0) & (samples < V)).all()), f'{what}: samples out of range: {samples[:8]}'
        u = u01(words(V, rowfield, seed, offset))
    worst, near = 0.0, 0
    for r in range(R):
        w = f'{what} row {r}'
        L, flag = live_set(xs[r], k)
        if flags is not None:
            want = flag if register else SENTINEL
            assert int(flags[r]) == want, f'{w}: row_flags {int(flags[r])}, expected {want}'
        if probs is None:
            if samples is None:
                continue
            j = int(samples[r])
            if filtered:                                    # (the engine: no probs_out) top-k alone has an exact kept set: race on it
                assert not topp_on(p), 'a top-p draw is certified on the kept set of its own probs_out'
                if not L.any():
                    continue
                assert L[j], f'{w}: drew column {j} outside the top-{k} set (logit {x[r, j]!r})'
                d, d2 = race_deficit(softmax64(xs[r], L)[0], u[r], j)
                assert d <= C_RACE, f'{w}: drew column {j} whose race score is {d:.1f} units below the best (C_RACE {C_RACE})'
                _note('race deficit', d)
                worst, near = max(worst, d), near + (d2 <= C_RACE)
                continue
            g = gumbel_scores(x[r], T, u[r])
            if not np.isfinite(g).any():
                continue                                    # nothing to draw from
            assert g[j] > -np.inf, f'{w}: drew column {j}, which is masked (logit {x[r, j]!r})'
            d, d2 = gumbel_deficit(g, j)
            assert d <= C_GUMBEL, f'{w}: drew column {j} whose Gumbel score is {d:.1f} units below the best (C_GUMBEL {C_GUMBEL})'
            _note('gumbel deficit', d)
            worst, near = max(worst, d), near + (d2 <= C_GUMBEL)
            continue
        if not L.any():
            continue                                        # a row of NaN / -inf: nothing is defined
        pr = probs[r]
        if topp_on(p):
            K = pr > 0
            check_topp(K, xs[r], L, V, p, w)
        else:
            K = L
        p64, a = softmax64(xs[r], K)
        check_probs(pr, p64, a, K, V, topp_on(p), w)
        if samples is None:
            continue
        j = int(samples[r])
        Kd = pr > 0                                         # teacher-forced: what the kernel itself could draw from
        assert Kd[j], f'{w}: drew column {j}, whose probability is 0 (logit {x[r, j]!r})'
        pd = softmax64(xs[r], Kd)[0] if not np.array_equal(Kd, K) else p64
        d, d2 = race_deficit(pd, u[r], j)
        assert d <= C_RACE, f'{w}: drew column {j} whose race score is {d:.1f} units below the best (C_RACE {C_RACE})'
        _note('race deficit', d)
        worst, near = max(worst, d), near + (d2 <= C_RACE)
    return worst, near


# ------------------------------------------------------------------------------------------------ the float32 model and the measurements
def model_probs32(xs, L, top_p=None, kept=None):
    """numpy float32 softmax over the live set (exp, sum, divide), then -- top_p given -- the oracle's top-p on the float32 values
    (stable descending sort, float32 cumsum, crossing token kept) and the second division"""
    f = np.float32
    z = np.where(L, xs, f(-np.inf)).astype(f)
    with np.errstate(invalid='ignore'):
        e = np.exp(z - z.max(), dtype=f)
    q = (e / e.sum(dtype=f)).astype(f)
    if topp_on(top_p):
        if kept is None:
            order = np.argsort(-q, kind='stable')
            cum = np.cumsum(q[order], dtype=f)
            n = int(np.searchsorted(cum, f(top_p), side='left')) + 1          # the first cum >= p is kept
            kept = np.zeros(len(q), bool)
            kept[order[:min(n, int(L.sum()))]] = True
        q = np.where(kept, q, f(0))
        q = (q / q.sum(dtype=f)).astype(f)
    return q


def model_race32(q, u):
    """the float32 race scores q / -log(u) (the draw is their argmax, lowest index on ties)"""
    f = np.float32
    with np.errstate(divide='ignore'):
        return (q / -np.log(u.astype(f), dtype=f)).astype(f)


def model_gumbel32(x, T, u):
    """the float32 Gumbel scores x * fl(1 / T) - log(-log u) as the streaming kernel forms them, NaN -> -inf"""
    f = np.float32
    with np.errstate(all='ignore'):
        g = (x.astype(f) * (f(1) / f(T))).astype(f)
        return (np.where(np.isnan(g), f(-np.inf), g) - np.log(-np.log(u.astype(f), dtype=f), dtype=f)).astype(f)


def measure_inputs():
    """(V, rows, T, k, p) of the reference-side measurement: N(0, 2.5) logits, seed 7, offset 5"""
    return [(64, 2048, 1.0, None, None), (64, 512, 1.0, 10, 0.9), (1000, 2048, 1.0, None, None), (1000, 512, 0.7, 50, 0.95),
            (1000, 512, 20.0, None, 0.5), (1000, 512, 0.05, None, None), (16384, 256, 1.0, None, None), (16384, 128, 1.0, 1024, 0.95)]


def gauss_logits(rows, V, seed, scale=2.5):
    return (scale * np.random.default_rng(seed).standard_normal((rows, V))).astype(np.float32)


def measure():
    """The reference-side measurement behind C_RACE and C_GUMBEL: over the rows of measure_inputs(), the largest error of the float32
    model's score of the two leading columns of the fp64 race (the only ones that can decide a draw) against their fp64 score, in
    units of u (race: of the best score; Gumbel: of max(1, |max g|)).  A draw decided by float32 scores that are each within d of the fp64
    ones falls short of the fp64 best by at most 2 d: C = 4 x the measurement.  Also counts the rows whose fp64 runner-up lies inside
    the tolerance, and the rows in which the float32 model draws another column than the fp64 race.
    -> (race, gumbel, rows, near_race, near_gumbel, swaps)"""
    race = gum = 0.0
    rows = near_r = near_g = swaps = 0
    for V, R, T, k, p in measure_inputs():
        x = gauss_logits(R, V, 1000 + V)
        xs, u = scaled(x, T), u01(words(V, np.arange(R), 7, 5))
        for r in range(R):
            L, _ = live_set(xs[r], k)
            q = model_probs32(xs[r], L, p)
            p64 = softmax64(xs[r], q > 0)[0]
            s32, s64 = model_race32(q, u[r]).astype(np.float64), p64 / -np.log(u[r])
            top = np.argsort(s64)[-2:]
            race = max(race, float(np.abs(s32[top] - s64[top]).max() / s64[top[1]] / U))
            g32, g64 = model_gumbel32(x[r], T, u[r]).astype(np.float64), gumbel_scores(x[r], T, u[r])
            gtop = np.argsort(g64)[-2:]
            gum = max(gum, float(np.abs(g32[gtop] - g64[gtop]).max() / (U * max(1.0, abs(g64[gtop[1]])))))
            d2, e2 = race_deficit(p64, u[r], int(top[1]))[1], gumbel_deficit(g64, int(gtop[1]))[1]
            rows, near_r, near_g = rows + 1, near_r + int(d2 <= C_RACE), near_g + int(e2 <= C_GUMBEL)
            swaps += int(np.argmax(s32) != top[1]) + int(np.argmax(g32) != gtop[1])
    return race, gum, rows, near_r, near_g, swaps


# ------------------------------------------------------------------------------------------------ buffers
def guarded_int(shape, dtype, device):
    """an integer output of `shape` inside a flat buffer with kernel_check.GUARD elements on either side, all SENTINEL: (buf, view)"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * kc.GUARD,), SENTINEL, dtype=dtype, device=device)
    return buf, buf[kc.GUARD:kc.GUARD + n].view(shape)


def check_guard_int(buf, n, what=''):
    for part, name in ((buf[:kc.GUARD], 'before'), (buf[kc.GUARD + n:], 'after')):
        bad = part != SENTINEL
        if bool(bad.any()):
            raise AssertionError(f'{what}: {int(bad.sum())} stores {name} the output (first at guard offset {int(bad.nonzero()[0, 0])})')


Call = collections.namedtuple('Call', 'samples probs flags status')


def call_scalar(nat, logits, T, k, p, seed, offset, want_probs=True, want_samples=True, want_flags=True, expect=0):
    """rqamd_sample_logits with caller-owned guarded buffers; logits: a device tensor (the front view of a poisoned buffer).  Returns
    numpy copies; the guards are checked here.  expect: the status code (outputs must be untouched when it is not 0)."""
    rows, V = logits.shape
    dev = logits.device
    sb, s = guarded_int((rows,), torch.int64, dev)
    fb, f = guarded_int((rows,), torch.int32, dev)
    pb, pr = kc.guarded((rows, V), torch.float32, dev)
    with nat.on_device_of(logits):
        rc = nat.lib().rqamd_sample_logits(nat.ptr(logits), rows, V, float(T), 0 if k is None else int(k), -1.0 if p is None else float(p),
                                           int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), nat.ptr(s) if want_samples else None,
                                           nat.ptr(pr) if want_probs else None, nat.ptr(f) if want_flags else None, nat.stream_of(logits))
    assert rc == expect, (rc, nat.lib().rqamd_last_error())
    return _collect(rc, sb, s, fb, f, pb, pr, want_samples, want_probs, want_flags)


def call_rows(nat, logits, T, K, P, seeds, seed, offset, want_probs=True, want_flags=True):
    """rqamd_sample_logits_rows with caller-owned guarded buffers; T, K, P, seeds: device tensors (seeds or None)"""
    rows, V = logits.shape
    dev = logits.device
    sb, s = guarded_int((rows,), torch.int64, dev)
    fb, f = guarded_int((rows,), torch.int32, dev)
    pb, pr = kc.guarded((rows, V), torch.float32, dev)
    with nat.on_device_of(logits):
        rc = nat.lib().rqamd_sample_logits_rows(nat.ptr(logits), rows, V, nat.ptr(T), nat.ptr(K), nat.ptr(P), nat.ptr(seeds),
                                                int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), nat.ptr(s),
                                                nat.ptr(pr) if want_probs else None, nat.ptr(f) if want_flags else None, nat.stream_of(logits))
    assert rc == 0, (rc, nat.lib().rqamd_last_error())
    return _collect(rc, sb, s, fb, f, pb, pr, True, want_probs, want_flags)


def _collect(rc, sb, s, fb, f, pb, pr, want_samples, want_probs, want_flags):
    if s.is_cuda:
        torch.cuda.synchronize(s.device)
    check_guard_int(sb, s.numel(), 'samples_out')
    check_guard_int(fb, f.numel(), 'row_flags')
    kc.check_guard(pb, pr.numel(), 'probs_out')
    if rc != 0 or not want_samples:
        assert bool((s == SENTINEL).all()), 'samples_out was written'
    if rc != 0 or not want_flags:
        assert bool((f == SENTINEL).all()), 'row_flags was written'
    if rc != 0 or not want_probs:
        kc.check_nan(pr, 'probs_out')
    return Call(s.cpu().numpy() if want_samples and rc == 0 else None, pr.cpu().numpy() if want_probs and rc == 0 else None,
                f.cpu().numpy() if want_flags and rc == 0 else None, rc)


def register_eligible(V, k):
    return topk_on(k, V) and V <= SMP_T * SMP_VPT and V % 4 == 0


def run_scalar_case(nat, x, T, k, p, seed, offset, device, what=''):
    """One case of tests/test_gpu_sampler.py through rqamd_sample_logits.  Filtered: once with row_flags (register kernel where
    eligible), once without (general kernel), both certified, supports and probabilities compared under the bounds, and the draws
    once more without probs_out, identical.  Unfiltered: the general kernel (probs_out) by the race certificate, the streaming kernel
    (no probs_out) by the Gumbel one.  Returns (largest deficit, rows inside the runner-up tolerance, flags or None)."""
    R, V = x.shape
    logits = kc.poisoned(torch.from_numpy(np.ascontiguousarray(x)).to(device))
    rowfield = np.arange(R)
    reg = register_eligible(V, k)
    a = call_scalar(nat, logits, T, k, p, seed, offset)
    worst, near = certify(x, T, k, p, a.probs, a.samples, rowfield, seed, offset, what + ' [flags]', a.flags, reg)
    b = call_scalar(nat, logits, T, k, p, seed, offset, want_flags=False)
    w2, n2 = certify(x, T, k, p, b.probs, b.samples, rowfield, seed, offset, what + ' [no flags]')
    worst, near = max(worst, w2), max(near, n2)
    if reg or topp_on(p):
        compare_forms(x, T, k, p, a.probs, b.probs, what)
    c = call_scalar(nat, logits, T, k, p, seed, offset, want_probs=False)
    if topk_on(k, V) or topp_on(p):
        assert np.array_equal(c.samples, a.samples), f'{what}: the draws change when probs_out is not asked for'
        assert c.flags is None or np.array_equal(c.flags, a.flags)
    else:
        w3, n3 = certify(x, T, k, p, None, c.samples, rowfield, seed, offset, what + ' [streaming]')
        worst, near = max(worst, w3), max(near, n3)
    d = call_scalar(nat, logits, T, k, p, seed, offset, want_samples=False)
    assert np.array_equal(d.probs.view(np.uint32), a.probs.view(np.uint32)), f'{what}: probs_out changes when no draw is asked for'
    return worst, near, a.flags


def compare_forms(x, T, k, p, pa, pb, what=''):
    """the two kernels' probabilities of one row differ by no more than their two bounds; without top-p their supports are equal (each
    was certified against the exact top-k set), with top-p each kept set was certified on its own"""
    xs = scaled(x, T)
    for r in range(x.shape[0]):
        L, _ = live_set(xs[r], k)
        if not L.any():
            continue
        Ka, Kb = pa[r] > 0, pb[r] > 0
        if not topp_on(p) or np.array_equal(Ka, Kb):
            p64, a = softmax64(xs[r], Ka if topp_on(p) else L)
            bound = prob_bound(p64, a, x.shape[1], topp_on(p))[0]
            err = np.abs(pa[r].astype(np.float64) - pb[r].astype(np.float64))
            assert (err <= 2 * bound).all(), f'{what} row {r}: the register and the general kernel differ by {err.max():.3e}'
        else:
            assert int((Ka ^ Kb).sum()) <= 1 + int((xs[r][L] == xs[r][Ka | Kb].min()).sum()), \
                f'{what} row {r}: the two kernels keep sets that differ in {int((Ka ^ Kb).sum())} columns'


def run_rows_case(nat, x, table, seeds, seed, offset, device, what=''):
    """rqamd_sample_logits_rows over the rows of x with table[r] = (T, k or None, p or None): every row certified against the reference
    with its own values -- row field r and key `seed`, or (seeds given) row field 0, key seeds[r] and offset `offset` -- once with
    probs_out (every row in the register or the general kernel) and once without (unfiltered rows: the streaming kernel's certificate;
    filtered rows: the same draw).  row_flags is written for the register kernel's rows alone."""
    R, V = x.shape
    logits = kc.poisoned(torch.from_numpy(np.ascontiguousarray(x)).to(device))
    T = torch.tensor([t for t, _, _ in table], dtype=torch.float32, device=device)
    K = torch.tensor([0 if k is None else k for _, k, _ in table], dtype=torch.int32, device=device)
    P = torch.tensor([-1.0 if p is None else p for _, _, p in table], dtype=torch.float32, device=device)
    S = None if seeds is None else torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64, device=device)
    a = call_rows(nat, logits, T, K, P, S, seed, offset)
    b = call_rows(nat, logits, T, K, P, S, seed, offset, want_probs=False)
    c = call_rows(nat, logits, T, K, P, S, seed, offset, want_flags=False)
    worst = near = 0
    for r, (t, k, p) in enumerate(table):
        field, key = ([r], seed) if seeds is None else ([0], seeds[r])
        w = f'{what} row {r} {table[r]}'
        reg = register_eligible(V, k)
        d, n = certify(x[r:r + 1], t, k, p, a.probs[r:r + 1], a.samples[r:r + 1], field, key, offset, w, a.flags[r:r + 1], reg)
        d2, n2 = certify(x[r:r + 1], t, k, p, c.probs[r:r + 1], c.samples[r:r + 1], field, key, offset, w + ' [no flags]')
        worst, near = max(worst, d, d2), near + max(n, n2)
        assert int(b.flags[r]) == int(a.flags[r]), w
        if topk_on(k, V) or topp_on(p):
            assert int(b.samples[r]) == int(a.samples[r]), f'{w}: the draw changes when probs_out is not asked for'
        else:
            d, n = certify(x[r:r + 1], t, k, p, None, b.samples[r:r + 1], field, key, offset, w + ' [streaming]')
            worst, near = max(worst, d), near + n
    return worst, near


def certify_engine(codes, logits, T, top_k, seed, offset, what=''):
    """Every code of an engine call is the certified winner of its step: codes (B, H, W, D) int64 numpy, logits (B, H, W, D, V) the
    teacher-forced (guided) logits of those codes with the LogitMask applied, top_k one value per depth (None or >= V: unfiltered, the
    streaming kernel; top-p off).  Step (pos, d) of image b draws from counter offset + pos D + d with row field b."""
    B, H, W, D = codes.shape
    worst = near = 0
    for pos in range(H * W):
        for d in range(D):
            x = logits.reshape(B, H * W, D, -1)[:, pos, d]
            j = codes.reshape(B, H * W, D)[:, pos, d]
            w, n = certify(x, T, top_k[d], None, None, j, np.arange(B), seed, offset + pos * D + d, f'{what} position {pos} depth {d}')
            worst, near = max(worst, w), near + n
    return worst, near


# ------------------------------------------------------------------------------------------------ cases
# kind: 'gauss' N(0, 2.5); 'distinct' a permutation of V distinct values; 'bucket<n>' n distinct values inside the bf16 bucket
# [1, 1.0078125) (one 16-bit key prefix) + 5 larger ones + smaller ones with other prefixes; 'negative' all below 0; 'zeros' 5 positive
# values, +0.0 and -0.0 alternating over two thirds of the row, negatives; 'hard' the rows of per_image_sampling_cases.kernel_logits
# (two-valued, NaN, constant); 'const'; 'two' / 'three' few-valued rows; 'dominant' one logit 30 above the rest; 'one' all but one
# column -inf; 'half' the upper half -inf (mask_logits).  emu: 1 the host emulator runs it too, 2 as a `slow` test.
Case = collections.namedtuple('Case', 'name V rows T k p kind emu seed offset', defaults=(1.0, None, None, 'gauss', 0, 7, 5))
P1 = float(np.nextafter(np.float32(1), np.float32(0)))
TOP_PS = (0.0, 1e-8, 0.5, 0.95, P1, 1.0)


def _cases():
    c = []
    for V in (4, 8, 500, 1024, 4096, 16384, 1, 7, 499, 1001, 16388, 16385):                 # register kernel; scalar loads; beyond the registers
        rows, emu = (64 if V <= 1024 else 16), int(V <= 1024)
        c.append(Case(f'V{V}_plain', V, rows, emu=emu))
        if V > 1:
            c.append(Case(f'V{V}_k_p', V, rows, 0.8, max(V // 8, 1), 0.9, emu=emu))
            c.append(Case(f'V{V}_kVm1', V, rows, 1.0, V - 1, None, emu=emu))
        c.append(Case(f'V{V}_k1', V, 8, 1.0, 1, None, emu=emu))
        c.append(Case(f'V{V}_kV_p', V, 8, 1.0, V, 0.5, emu=emu))
    c.append(Case('V36000_plain', 36000, 8))
    c.append(Case('V36000_k_p', 36000, 8, 0.9, 1000, 0.95))
    c.append(Case('cap_2048', 4096, 8, 1.0, 2048, 0.95, 'distinct', emu=2))                 # total == SMP_CAP: stays in the register kernel
    c.append(Case('cap_2049', 4096, 8, 1.0, 2049, 0.95, 'distinct', emu=2))                 # total == SMP_CAP + 1: handed back
    c.append(Case('bucket256', 1024, 8, 1.0, 133, None, 'bucket256', emu=1))               # und_n == SMP_UND: one wavefront settles
    c.append(Case('bucket257', 1024, 8, 1.0, 133, None, 'bucket257', emu=1))               # und_n == SMP_UND + 1: block-wide fallback
    c.append(Case('bucket256_p', 1024, 8, 1.0, 200, 0.9, 'bucket256', emu=1))
    c.append(Case('bucket257_p', 1024, 8, 1.0, 200, 0.9, 'bucket257', emu=1))
    c.append(Case('bucket_all', 1024, 8, 1.0, 100, None, 'bucket1024', emu=1))
    c.append(Case('negative', 500, 16, 1.0, 20, 0.9, 'negative', emu=1))
    c.append(Case('zeros_k', 500, 8, 1.0, 100, None, 'zeros', emu=1))                      # the threshold is +-0.0
    c.append(Case('zeros_k_p', 500, 8, 1.0, 100, 0.9, 'zeros', emu=1))
    c.append(Case('hard_k10', 500, 12, 1.0, 10, None, 'hard', emu=1))
    c.append(Case('hard_k10_p', 500, 12, 0.8, 10, 0.9, 'hard', emu=1))
    c.append(Case('hard_k10_V16384', 16384, 12, 1.0, 10, None, 'hard'))                     # the two-valued row ties past SMP_CAP
    for p, tag in zip(TOP_PS, ('0', '1em8', '0_5', '0_95', 'below1', '1')):
        c.append(Case(f'p{tag}', 500, 16, 1.0, None, p, emu=1))
        c.append(Case(f'p{tag}_k50', 500, 16, 1.0, 50, p, emu=1))
        c.append(Case(f'p{tag}_V16388', 16388, 8, 1.0, None, p))                            # the general kernel's LDS path
    for kind in ('const', 'two', 'three', 'dominant'):
        c.append(Case(f'{kind}_p', 500, 8, 1.0, None, 0.7, kind, emu=1))
        c.append(Case(f'{kind}_k_p', 500, 8, 1.0, 40, 0.7, kind, emu=1))
    c.append(Case('two_p_V16388', 16388, 8, 1.0, None, 0.7, 'two'))
    for kind in ('one', 'half'):
        c.append(Case(f'mask_{kind}', 500, 16, 1.0, None, None, kind, emu=1))
        c.append(Case(f'mask_{kind}_k_p', 500, 16, 1.0, 50, 0.9, kind, emu=1))
        c.append(Case(f'mask_{kind}_V499', 499, 16, 1.0, None, 0.9, kind, emu=1))
    for T in (0.05, 20.0):
        tag = ('%g' % T).replace('.', '_')
        c.append(Case(f'T{tag}', 1024, 32, T, emu=1))
        c.append(Case(f'T{tag}_k_p', 1024, 32, T, 100, 0.95, emu=1))
        c.append(Case(f'T{tag}_V16388', 16388, 8, T, None, 0.95))
    return c


CASES = _cases()
SEEDS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 11)
OFFSETS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3)
STREAM_ROWS = 300


def stream_cases(V, filtered_rows=STREAM_ROWS):
    """every seed x every offset over STREAM_ROWS rows, alternating between an unfiltered and a filtered draw (filtered_rows: the
    emulator's fibers need a second per filtered row, so its filtered cases run fewer)"""
    out = []
    for i, s in enumerate(SEEDS):
        for j, o in enumerate(OFFSETS):
            k, p = ((None, None), (V // 8, 0.9))[(i + j) % 2]
            out.append(Case(f'seed{s:x}_offset{o:x}', V, STREAM_ROWS if k is None else filtered_rows, 1.0, k, p, seed=s, offset=o))
    return out


def build_logits(case):
    """the (rows, V) float32 logits of a case, from its name alone"""
    R, V, kind = case.rows, case.V, case.kind
    rng = np.random.default_rng(sum(case.name.encode()) * 7919 + V)
    x = (2.5 * rng.standard_normal((R, V))).astype(np.float32)
    if kind == 'distinct':
        base = np.linspace(-6.0, 6.0, V).astype(np.float32)
        assert len(np.unique(base)) == V
        x = np.stack([rng.permutation(base) for _ in range(R)])
    elif kind.startswith('bucket'):
        n = int(kind[6:])
        for r in range(R):
            inb = (np.float32(1.0).view(np.uint32) + rng.choice(2 ** 16, n, replace=False).astype(np.uint32)).view(np.float32)
            rest = np.clip(x[r, :V - n], -9.0, 0.98).astype(np.float32)
            rest[:min(5, len(rest))] = np.arange(2, 2 + min(5, len(rest)), dtype=np.float32)
            x[r] = rng.permutation(np.concatenate([inb, rest]))
    elif kind == 'negative':
        x = -np.abs(x) - np.float32(0.1)
    elif kind == 'zeros':
        neg = -np.abs(x) - np.float32(0.1)
        for r in range(R):
            row = neg[r].copy()
            z = rng.permutation(V)[:2 * V // 3 + 5]
            row[z[5::2]], row[z[6::2]] = np.float32(0.0), np.float32(-0.0)
            row[z[:5]] = np.arange(1, 6, dtype=np.float32)
            x[r] = row
    elif kind == 'hard':
        import per_image_sampling_cases as P
        x = P.kernel_logits(V, V)[:R]
    elif kind == 'const':
        x[:] = np.float32(0.25)
    elif kind == 'two':
        x = rng.choice([0.5, 1.5], (R, V), p=[0.4, 0.6]).astype(np.float32)
    elif kind == 'three':
        x = rng.choice([-1.0, 0.5, 1.5], (R, V)).astype(np.float32)
    elif kind == 'dominant':
        x[np.arange(R), rng.integers(0, V, R)] += np.float32(30.0)
    elif kind == 'one':
        keep = rng.integers(0, V, R)
        y = np.full((R, V), -np.inf, np.float32)
        y[np.arange(R), keep] = x[np.arange(R), keep]
        x = y
    elif kind == 'half':
        x[:, V // 2:] = -np.inf
    return np.ascontiguousarray(x, dtype=np.float32)


# The probe row: a draw that tells u = (2 (r >> 9) + 1) 2^-24 from any mapping that differs from it at a word below 64 (u = r / 2^32,
# say, which draws the same column as the kernel's u in all ordinary rows).  Found by searching the reference stream: with seed 7 and
# offset 33871185, counter (0, 0, offset) holds the word 15 at index 0.  The kernel's u there is 2^-24, E = -log u = 16.64; r / 2^32
# gives E = 19.47.  Columns 0 and 1 are live, with logits that make column 0 lead the race by 5 % (and the Gumbel scores by log 1.05)
# under the kernel's u and trail by 10 % under the other.
PROBE = dict(seed=7, offset=33871185, index=0, word=15)


def probe_logits():
    """-> (x (1, 4) float32, seed, offset)"""
    u = u01(words(4, [0], PROBE['seed'], PROBE['offset']))[0]
    E = -np.log(u)
    x = np.full((1, 4), -np.inf, np.float32)
    x[0, 1] = 0.0
    x[0, 0] = np.float32(np.log(1.05 * E[0] / E[1]))
    return x, PROBE['seed'], PROBE['offset']
