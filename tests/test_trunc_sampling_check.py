"""CPU-only evidence that the certificates of tests/trunc_sampling_cases.py can fail, and their power.  A numpy-float32 model of the
whole chain (top-k, softmax, top-p, min-p, typical, exponential race) is accepted as it stands and rejected under each mutation: a
typical set with one token too many, one too few, the wrong member of a tie, a token from the far side of the order swapped in, and a
min-p set that misses an entry 1 % above the threshold (or holds one 1 % below).  Also here: the probability bound against
sampler_check's at one and two divisions, the reference-side measurement behind C_RACE_T, and the power conditions -- no entry inside
the min-p band in at least 99 % of rows, exactly one legitimate prefix of the typical order in at least 90 % of the tie-free rows of
each Gaussian case, the race runner-up inside the tolerance in fewer than 1 % of rows."""
import numpy as np
import pytest

import sampler_check as sc
import trunc_sampling_cases as tc

SEED, OFFSET = 2 ** 63 + 2 ** 32 + 11, 2 ** 40 + 3
f32 = np.float32


def case(name, rows=16):
    c = next(c for c in tc.CASES if c.name == name)
    return c._replace(rows=min(c.rows, rows))


def model_calls(x, T, k, p, mp, ty, mut=None):
    """the three calls of the chain by the float32 model -> (Stage, samples of the last)"""
    R, V = x.shape
    xs = sc.scaled(x, T)
    u = sc.u01(sc.words(V, np.arange(R), SEED, OFFSET))
    p1 = np.stack([tc.model_chain32(xs[r], k, p, None, None) for r in range(R)])
    p2 = np.stack([tc.model_chain32(xs[r], k, p, mp, None, mut) for r in range(R)]) if tc.minp_on(mp) else None
    p3 = np.stack([tc.model_chain32(xs[r], k, p, mp, ty, mut) for r in range(R)]) if tc.typ_on(ty) else None
    last = p3 if p3 is not None else p2
    samples = np.array([int(np.argmax(sc.model_race32(np.nan_to_num(last[r]), u[r]))) for r in range(R)], np.int64)
    return tc.Stage(p1, p2, p3), samples


def judge(c, mut=None, x=None):
    x = tc.build_logits(c) if x is None else x
    st, samples = model_calls(x, c.T, c.k, c.p, c.min_p, c.typ, mut)
    return tc.certify_chain(x, c.T, c.k, c.p, c.min_p, c.typ, st, samples, np.arange(x.shape[0]), SEED, OFFSET, f'{c.name} / {mut}')


ACCEPTED = ('V500_koff_minp', 'V500_koff_typ', 'V500_k62_all', 'V499_koff_minp_typ', 'V7_koff_all', 'V1_koff_all', 'minp1', 'minp1em08_k50',
            'typ0', 'typ1em08_k50', 'typbelow1', 'const_typ', 'const_k_all', 'two_typ', 'three_k_all', 'dominant_typ', 'one_typ', 'half_k_all',
            'hard_k_all', 'negative_typ', 'T0_05_all', 'T20_all')


@pytest.mark.parametrize('name', ACCEPTED)
def test_model_is_accepted(name):
    judge(case(name))


# mutation -> the case it is shown on
MUTATIONS = {
    'typ_long': 'V500_koff_typ',           # one token too many
    'typ_short': 'V500_koff_typ',          # one token too few
    'typ_high_ties': 'two_typ',            # the wrong member of a tie
    'typ_swap': 'V500_k62_all',            # a token from the far side of the order in place of the boundary token
    'minp_long': 'V500_koff_minp',         # the best dropped entry kept
    'minp_short': 'V500_koff_minp',        # the smallest kept entry dropped
}


@pytest.mark.parametrize('mut', sorted(MUTATIONS))
def test_mutation_is_rejected(mut):
    with pytest.raises(AssertionError) as e:
        judge(case(MUTATIONS[mut]), mut)
    print(f'{mut}: rejected on {MUTATIONS[mut]}: {str(e.value)[:160]}')


def _threshold_rows(rel):
    """rows of 64 logits whose column 5 has rel x min_p x the leader's probability (min_p = 0.5, the leader in column 0)"""
    rng = np.random.default_rng(3)
    x = (-6.0 - np.abs(rng.standard_normal((8, 64)))).astype(f32)
    x[:, 0] = 2.0
    x[:, 1:4] = [1.8, 1.7, 1.5]
    x[:, 5] = f32(2.0 + np.log(0.5 * rel))
    return x


def test_min_p_one_percent_above_the_threshold_must_be_kept():
    """the certificate rejects a min-p set that misses an entry 1 % above the threshold, and one that holds an entry 1 % below"""
    c = tc.Case('threshold', 64, 8, 1.0, None, None, 0.5, None)
    for rel, mut in ((1.01, 'minp_short'), (0.99, 'minp_long')):
        x = _threshold_rows(rel)
        xs = sc.scaled(x, 1.0)
        assert all(tc.reference_sets(xs[r], None, None, 0.5, None)[2][5] == (rel > 1) for r in range(8))
        judge(c, None, x)
        with pytest.raises(AssertionError, match='threshold'):
            judge(c, mut, x)
        # the set itself, whatever produced it
        P = np.ones(64, bool)
        K = tc.reference_sets(xs[0], None, None, 0.5, None)[2].copy()
        tc.check_minp(K, xs[0], P, 64, 0.5, 1)
        K[5] = not K[5]
        with pytest.raises(AssertionError, match='threshold'):
            tc.check_minp(K, xs[0], P, 64, 0.5, 1)
    print('min-p: an entry 1 % above the threshold cannot be dropped, one 1 % below cannot be kept')


def test_typical_sets_one_off_are_rejected_directly():
    """the typical certificate on sets built from the fp64 reference: the reference's set passes; one token more, one token less, the
    last token of the order swapped in, and the higher index of a tie each fail"""
    c = case('V500_koff_typ')
    xs = sc.scaled(tc.build_logits(c), c.T)
    rejected = {'long': 0, 'short': 0, 'swap': 0}
    for r in range(c.rows):
        _, _, K2, K3 = tc.reference_sets(xs[r], None, None, None, c.typ)
        tc.check_typical(K3, xs[r], K2, c.V, c.typ, 1)
        order = tc.typical_order(tc.typical_terms(xs[r], K2, c.V, 1)[2], K2)
        n = int(K3.sum())
        assert set(order[:n]) == set(np.flatnonzero(K3)) and 1 < n < len(order)
        for name, ids in (('long', order[:n + 1]), ('short', order[:n - 1]), ('swap', np.concatenate([order[:n - 1], order[-1:]]))):
            K = np.zeros_like(K3)
            K[ids] = True
            try:
                tc.check_typical(K, xs[r], K2, c.V, c.typ, 1)
            except AssertionError:
                rejected[name] += 1
    print(f'typical, {c.rows} rows: rejected {rejected}')
    assert rejected['swap'] == c.rows and rejected['long'] >= c.rows - 1 and rejected['short'] >= c.rows - 1
    c = case('two_typ')
    xs = sc.scaled(tc.build_logits(c), c.T)
    for r in range(c.rows):
        _, _, K2, K3 = tc.reference_sets(xs[r], None, None, None, c.typ)
        tc.check_typical(K3, xs[r], K2, c.V, c.typ, 1)
        b = int(np.flatnonzero(K3)[-1])
        same = np.flatnonzero(K2 & ~K3 & (xs[r] == xs[r][b]))
        if len(same):
            K = K3.copy()
            K[b], K[same[-1]] = False, True
            with pytest.raises(AssertionError, match='lowest indices'):
                tc.check_typical(K, xs[r], K2, c.V, c.typ, 1)


def test_probability_bound_extends_the_sampler_bound():
    rng = np.random.default_rng(0)
    xs = (2.5 * rng.standard_normal(500)).astype(f32)
    p64, a = sc.softmax64(xs, np.ones(500, bool))
    for ndiv, two in ((1, False), (2, True)):
        assert np.array_equal(tc.prob_bound(p64, a, 500, ndiv)[0], sc.prob_bound(p64, a, 500, two)[0])
    assert tc.prob_bound(p64, a, 500, 4)[1] == tc.prob_bound(p64, a, 500, 2)[1] + 4


def test_reference_chain_semantics():
    """the fp64 reference on rows worked out by hand"""
    xs = np.log(np.array([0.5, 0.25, 0.125, 0.0625, 0.0625], np.float64)).astype(f32)
    _, K1, K2, K3 = tc.reference_sets(xs, None, None, 0.2, None)
    assert K2.tolist() == [True, True, True, False, False]                       # 0.125 >= 0.2 * 0.5, 0.0625 is not
    # H = 1.875 bits; surprisals 1, 2, 3, 4, 4 bits: |s - H| = 0.875, 0.125, 1.125, 2.125, 2.125 -> order 1, 0, 2, 3, 4
    _, _, _, K3 = tc.reference_sets(xs, None, None, None, 0.0)
    assert K3.tolist() == [False, True, False, False, False]
    _, _, _, K3 = tc.reference_sets(xs, None, None, None, 0.7)
    assert K3.tolist() == [True, True, False, False, False]                      # 0.25 + 0.5 = 0.75 >= 0.7
    _, _, _, K3 = tc.reference_sets(xs, None, None, None, 0.9)
    assert K3.tolist() == [True, True, True, True, False]                        # 0.875 < 0.9: the lower index of the tie comes next
    one = np.array([-np.inf, 1.0, -np.inf], f32)
    assert tc.reference_sets(one, None, None, 1.0, 0.5)[3].tolist() == [False, True, False]
    const = np.zeros(8, f32)
    assert tc.reference_sets(const, None, None, None, 0.3)[3].tolist() == [True] * 3 + [False] * 5


# ------------------------------------------------------------------------------------------------ constants and power
def test_measured_constant_and_draw_power():
    race, rows, near = tc.measure()
    print(f'float32 chain model against fp64 over {rows} rows: race {race:.3f} u (C_RACE_T {tc.C_RACE_T}); runner-up inside the tolerance: {near} rows')
    assert race <= tc.RACE_T_MEASURED and tc.C_RACE_T == 4.0 * tc.RACE_T_MEASURED
    assert race > 0.5 * tc.RACE_T_MEASURED                                        # (the constant is not stale)
    assert near < 0.01 * rows


def test_min_p_power():
    """no entry lies inside the tolerance band of the threshold in at least 99 % of the rows of the Gaussian cases"""
    rows = clean = 0
    for c in tc.CASES:
        if c.kind != 'gauss' or not tc.minp_on(c.min_p) or c.min_p >= 1.0:
            continue
        xs = sc.scaled(tc.build_logits(c), c.T)
        for r in range(c.rows):
            _, K1, K2, _ = tc.reference_sets(xs[r], c.k, c.p, c.min_p, None)
            rows, clean = rows + 1, clean + (tc.check_minp(K2, xs[r], K1, c.V, c.min_p, tc.n_div(c.p)) == 0)
    print(f'min-p: no entry inside the band in {clean} of {rows} rows')
    assert rows > 500 and clean >= 0.99 * rows


def test_typical_power():
    """exactly one prefix of the (a, index) order satisfies the mass condition in at least 90 % of the rows of each Gaussian case (the
    first rows of the case's own generator, 48 of them from V = 4096 up; rows with tied logits included, the index rule orders them).
    Not asked of typical_p = 1 - 2^-24: the tolerance of any mass certificate exceeds what the smallest tokens weigh, so nothing pins
    a cut there -- those cases are certified for legitimacy alone."""
    total, free, worst = 0, 0, 1.0
    for c in tc.CASES:
        if c.kind != 'gauss' or not tc.typ_on(c.typ) or c.typ >= sc.P1 or c.V < 64:
            continue
        c = c._replace(rows=48 if c.V > 1024 else c.rows)
        xs = sc.scaled(tc.build_logits(c), c.T)
        rows = one = 0
        for r in range(c.rows):
            _, _, K2, _ = tc.reference_sets(xs[r], c.k, c.p, c.min_p, None)
            if int(K2.sum()) < 2:
                continue
            free += len(np.unique(xs[r][K2])) == int(K2.sum())
            rows, one = rows + 1, one + (tc.typical_prefix_count(xs[r], K2, c.V, c.typ, tc.n_div(c.p, c.min_p)) == 1)
        if rows:
            print(f'{c.name}: exactly one legitimate prefix in {one} of {rows} rows')
            assert one >= 0.9 * rows, c.name
            total, worst = total + rows, min(worst, one / rows)
    print(f'typical: {total} rows ({free} of them tie-free), the weakest case pins {100 * worst:.1f} % of its rows')
    assert total > 500
