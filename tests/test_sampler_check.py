"""CPU-only evidence that the checks of tests/sampler_check.py can fail: a numpy-float32 model of the sampler (Philox stream, top-k,
softmax, top-p, exponential race / Gumbel-max, stores into guarded buffers) is accepted as it stands and rejected under each of the
mutations below, by the checks the GPU and emulator tests run on the real kernels.  Also here: the Philox known answers, the
reference-side measurement behind C_RACE / C_GUMBEL, and the two power conditions (the runner-up lies inside the draw tolerance in
fewer than 1 % of rows; exactly one sorted prefix satisfies the top-p mass condition in at least 95 % of tie-free rows)."""
import numpy as np
import pytest
import torch

import kernel_check as kc
import sampler_check as sc

SEED, OFFSET = 2 ** 63 + 2 ** 32 + 11, 2 ** 40 + 3          # high words set in both
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the model
def model_words(V, rowfield, seed, offset, mut):
    R = len(rowfield)
    if mut == 'rounds9':
        return sc.words(V, rowfield, seed, offset, rounds=9)
    if mut == 'no_row':
        return sc.words(V, np.zeros(R, np.int64), seed, offset)
    if mut == 'offset_lo':
        return sc.words(V, rowfield, seed, offset & 0xFFFFFFFF)
    if mut == 'seed_lo':
        return sc.words(V, rowfield, seed & 0xFFFFFFFF, offset)
    w = sc.words(V + (-V) % 4, rowfield, seed, offset)
    if mut == 'word_perm':
        w = w.reshape(R, -1, 4)[:, :, [1, 0, 3, 2]].reshape(R, -1)
    return w[:, :V]


def model_u(w, mut):
    if mut == 'u_r32':
        return (w.astype(f32) / f32(2.0 ** 32)).astype(np.float64)            # u = r / 2^32: 0 and 1 are reachable, another grid
    return sc.u01(w)


def model(x, T, k, p, rowfield, seed=SEED, offset=OFFSET, mut=None, streaming=False):
    """-> (probs (R, V) float32 or None for the streaming form, samples (R,) int64)"""
    R, V = x.shape
    xs = sc.scaled(x, T)
    u = model_u(model_words(V, rowfield, seed, offset, mut), mut)
    probs, samples = np.zeros((R, V), f32), np.zeros(R, np.int64)
    for r in range(R):
        if streaming:
            g = sc.model_gumbel32(x[r], T, u[r])
            j = int(np.argmax(g))
            if mut == 'draw_masked' and np.isneginf(g).any():
                j = int(np.flatnonzero(np.isneginf(g))[0])
            samples[r] = j
            continue
        L, _ = sc.live_set(xs[r], k)
        if sc.topk_on(k, V):
            kth = sc.kth_largest(xs[r], k)
            if mut == 'topk_gt':
                L = L & (xs[r] > kth)
            if mut == 'topk_drop_negzero' and kth == 0:
                L = L & ~((xs[r] == 0) & np.signbit(xs[r]))
        kept = None
        if sc.topp_on(p) and mut in ('topp_short', 'topp_long', 'topp_high_ties'):
            q = sc.model_probs32(xs[r], L)
            order = np.argsort(-q, kind='stable')
            if mut == 'topp_high_ties':
                order = (V - 1 - np.argsort(-q[::-1], kind='stable'))           # highest index first among equals
            n = int(np.searchsorted(np.cumsum(q[order], dtype=f32), f32(p), side='left')) + 1
            n = {'topp_short': max(n - 1, 1), 'topp_long': n + 1, 'topp_high_ties': n}[mut]
            kept = np.zeros(V, bool)
            kept[order[:min(n, int(L.sum()))]] = True
        q = sc.model_probs32(xs[r], L, p, kept)
        if mut == 'no_renorm' and sc.topp_on(p):
            q1 = sc.model_probs32(xs[r], L)
            q = np.where(q > 0, q1, f32(0))
        if mut == 'prob_off':
            K = q > 0
            p64, a = sc.softmax64(xs[r], K)
            i = int(np.argmax(q))
            q = q.copy()
            q[i] = f32(q[i] + 4.0 * sc.prob_bound(p64, a, V, sc.topp_on(p))[0][i])
        probs[r] = q
        s = sc.model_race32(q, u[r])
        if mut == 'race_times':
            with np.errstate(divide='ignore'):
                s = (q * -np.log(u[r].astype(f32), dtype=f32)).astype(f32)                  # argmax p * E
        j = int(np.argmax(s))
        if mut == 'second_best':
            j = int(np.argsort(s, kind='stable')[-2])
        if mut == 'draw_masked' and (q == 0).any():
            j = int(np.flatnonzero(q == 0)[0])
        samples[r] = j
    return (None if streaming else probs), samples


def case(name):
    c = next(c for c in sc.CASES if c.name == name)
    return c._replace(rows=min(c.rows, 32))


def judge(c, mut=None, streaming=False, seed=SEED, offset=OFFSET):
    x = sc.build_logits(c)
    rowfield = np.arange(c.rows)
    probs, samples = model(x, c.T, c.k, c.p, rowfield, seed, offset, mut, streaming)
    return sc.certify(x, c.T, c.k, c.p, probs, samples, rowfield, seed, offset, f'{c.name} / {mut}')


# mutation -> (the case it is shown on, streaming form too)
MUTATIONS = {
    'rounds9': ('V500_plain', True),                 # 9 Philox rounds
    'word_perm': ('V500_plain', True),               # words index % 4 permuted
    'no_row': ('V500_plain', True),                  # row field ignored
    'offset_lo': ('V500_plain', True),               # high word of the offset dropped
    'seed_lo': ('V500_plain', True),                 # high word of the seed dropped
    'race_times': ('V500_k_p', False),               # argmax p * E
    'second_best': ('V500_k_p', False),              # second-best pick
    'draw_masked': ('mask_half', True),              # a -inf column drawn
    'topk_gt': ('three_k_p', False),                 # top-k with >
    'topk_drop_negzero': ('zeros_k', False),         # top-k dropping -0.0
    'topp_short': ('V500_k_p', False),               # top-p without the crossing token
    'topp_long': ('V500_k_p', False),                # top-p with one token too many
    'topp_high_ties': ('two_p', False),              # highest-index ties
    'no_renorm': ('V500_k_p', False),                # no renormalisation
    'prob_off': ('V500_k_p', False),                 # one probability off by 4 bound-widths
}


@pytest.mark.parametrize('name', sorted({v[0] for v in MUTATIONS.values()} | {'zeros_k_p', 'p0', 'p1em8_k50', 'T0_05_k_p', 'hard_k10_p', 'const_p'}))
def test_model_is_accepted(name):
    c = case(name)
    judge(c)
    if not (sc.topk_on(c.k, c.V) or sc.topp_on(c.p)):
        judge(c, streaming=True)


@pytest.mark.parametrize('mut', sorted(MUTATIONS))
def test_mutation_is_rejected(mut):
    name, streaming = MUTATIONS[mut]
    with pytest.raises(AssertionError):
        judge(case(name), mut)
    print(f'{mut}: rejected on {name}')
    if streaming:
        with pytest.raises(AssertionError):
            judge(case(name), mut, streaming=True)
        print(f'{mut}: rejected on {name} (streaming form)')


def test_uniform_mutation_is_rejected_on_the_probe_row():
    """u = r / 2^32 draws what the kernel's u draws in all but ~1 of 2000 flat rows of 36000 columns, so no batch of ordinary rows shows
    it.  The probe row (sampler_check.PROBE, found by searching the reference stream) holds a word below 64, where the kernel's u is
    2^-24 and r / 2^32 is at least four times smaller: its two live logits are set so that the draw tells the two apart."""
    x, seed, offset = sc.probe_logits()
    w = sc.words(x.shape[1], [0], seed, offset)
    assert int(w[0, sc.PROBE['index']]) == sc.PROBE['word'] < 64
    for streaming in (False, True):
        probs, samples = model(x, 1.0, None, None, [0], seed, offset, None, streaming)
        sc.certify(x, 1.0, None, None, probs, samples, [0], seed, offset, 'probe')
        probs, samples = model(x, 1.0, None, None, [0], seed, offset, 'u_r32', streaming)
        with pytest.raises(AssertionError):
            sc.certify(x, 1.0, None, None, probs, samples, [0], seed, offset, 'probe / u_r32')
    print('u_r32: rejected on the probe row, both forms')


def test_store_past_samples_out_is_rejected():
    buf, view = sc.guarded_int((12,), torch.int64, 'cpu')
    view[:] = 3
    sc.check_guard_int(buf, 12)
    buf[kc.GUARD + 12] = 3                                  # one element past samples_out
    with pytest.raises(AssertionError):
        sc.check_guard_int(buf, 12, 'samples_out')
    buf, view = sc.guarded_int((12,), torch.int32, 'cpu')
    buf[kc.GUARD - 1] = 0
    with pytest.raises(AssertionError):
        sc.check_guard_int(buf, 12, 'row_flags')


# ------------------------------------------------------------------------------------------------ known answers
def test_philox_known_answers():
    """Philox4x32-10 of the Random123 distribution (kat_vectors): zero counter and key; all-ones counter and key; the digits of pi"""
    assert [int(v) for v in sc.philox4x32(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    m = 0xffffffff
    assert [int(v) for v in sc.philox4x32(m, m, m, m, m, m)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    got = sc.philox4x32(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)
    assert [int(v) for v in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_uniform_grid():
    """u = (2 (r >> 9) + 1) 2^-24: exact in float32, strictly inside (0, 1), the extremes 2^-24 and 1 - 2^-24"""
    w = np.array([0, 511, 512, 2 ** 32 - 1, 2 ** 32 - 512, 0x80000000], dtype=np.uint64)
    u = sc.u01(w)
    assert u.tolist() == [2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24, 1 - 2.0 ** -24, 1 - 2.0 ** -24, 0.5 + 2.0 ** -24]
    assert np.array_equal(u.astype(f32).astype(np.float64), u)
    # the counter layout: word i of a row comes from counter i / 4, and the row, offset and seed words each matter
    a = sc.words(9, [0, 1], 7, 5)
    assert not np.array_equal(a[0], a[1])
    for other in (sc.words(9, [0, 1], 7 + 2 ** 32, 5), sc.words(9, [0, 1], 7, 5 + 2 ** 32), sc.words(9, [0, 1], 7, 6)):
        assert not (a == other).any()
    assert [int(v) for v in a[1, 4:8]] == [int(v) for v in sc.philox4x32(1, 1, 5, 0, 7, 0)]


# ------------------------------------------------------------------------------------------------ constants and power
def test_measured_constants_and_draw_power():
    race, gum, rows, near_r, near_g, swaps = sc.measure()
    print(f'float32 model against fp64 over {rows} rows: race {race:.3f} u (C_RACE {sc.C_RACE}), Gumbel {gum:.3f} u (C_GUMBEL {sc.C_GUMBEL}); '
          f'runner-up inside the tolerance: {near_r} / {near_g} rows; draws that differ from the fp64 race: {swaps}')
    assert race <= sc.RACE_MEASURED and sc.C_RACE == 4.0 * sc.RACE_MEASURED
    assert gum <= sc.GUMBEL_MEASURED and sc.C_GUMBEL == 4.0 * sc.GUMBEL_MEASURED
    assert race > 0.5 * sc.RACE_MEASURED and gum > 0.5 * sc.GUMBEL_MEASURED          # (the constants are not stale)
    assert near_r < 0.01 * rows and near_g < 0.01 * rows


def test_top_p_power():
    """on the tie-free cases exactly one sorted prefix satisfies the mass condition in at least 95 % of rows"""
    rows = one = 0
    for c in sc.CASES:
        if c.kind != 'gauss' or not sc.topp_on(c.p) or c.p == 0.0 or c.V > 4096:
            continue
        xs = sc.scaled(sc.build_logits(c), c.T)
        for r in range(c.rows):
            L, _ = sc.live_set(xs[r], c.k)
            if len(np.unique(xs[r][L])) < int(L.sum()):
                continue
            rows, one = rows + 1, one + (sc.prefix_count(xs[r], L, c.V, c.p) == 1)
    print(f'top-p: exactly one legitimate prefix in {one} of {rows} tie-free rows')
    assert rows > 500 and one >= 0.95 * rows
