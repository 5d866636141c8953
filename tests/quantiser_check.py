"""Certificate checks of the residual quantiser (csrc/quantize.hip) against fp64, shared by tests/test_gpu_quantiser.py (the MI355X),
tests/test_emu_quantiser.py (the host emulator) and tests/test_quantiser_check.py (the evidence that these checks can fail).  No GPU
dependency: everything here is torch / numpy on whatever device the tensors live on.

Per depth, teacher-forced on the kernel's own codes: the residual r_d = x - c[code_0] - ... - c[code_{d-1}] formed by elementwise fp32
subtractions is bit-identical to the kernel's, so nothing drifts.  From the fp32 residual r and codebook c, in fp64:

    d64 = |r|^2 + |c|^2 - 2 r.c            S = |r|^2 + |c|^2 + 2 |r|.|c|   (absolute values termwise)

The kernel's distance fmaf(-2, acc, xn + cn) is built from xn (dim / 8 + 3 sequential fp32 roundings: <= (dim / 8 + 3) u |r|^2), cn
(dim / 4 + 2 roundings: <= (dim / 4 + 2) u |c|^2), acc (an fmaf chain of dim steps on v_mfma_f32_32x32x2_f32: <= dim u |r|.|c|) and two
final roundings, so to first order

    |d_kernel - d64| <= E := c u n S,     u = 2^-24, n = dim + 4,     c = 1  (derived, not measured: the ceiling of every check)

 1. code certificate (every vector, every depth, nothing left out): the kernel chose k because ITS distance to k was minimal, hence
    d64[k] - E[k] <= min_j (d64[j] + E[j]).  A failure is a wrong code, never noise.
 2. certificate power (a condition on the inputs): the share of (vector, depth) pairs in which a second code satisfies the same
    inequality -- asserted <= 1 % per case by the tests, else the certificate would not pin the code.
 3. ties: a code must be the lowest index among the codebook rows bit-equal to it (torch.argmin's first minimum).
 4. quants: quant_cum[d] is the depth-ordered fp32 sum of c[code], bit for bit (sequential loop), as are rq_embed modes 0 / 1 / 2.
 5. distance values: |d - d64| <= c u n S elementwise with c = 1, and with the tighter C_CHAIN below.
 6. soft codes: |soft - p64| <= p64 (expm1(2 max_j E_j / temp) + KAPPA) + 2^-126 against the fp64 softmax of -d64 / temp; rows sum
    to 1 within K u.
 7. code norms: |cn - cn64| <= (dim / 4 + 2) u cn64.
 8. memory: inputs are the front views of NaN-filled buffers (kernel_check.poisoned), outputs views into guard-filled buffers
    (kernel_check.guarded for fp32, guarded_codes here for the int64 codes: -1), no code < 0 or >= K."""
import collections
import math

import numpy as np
import torch

import kernel_check as kc

U = 2.0 ** -24                 # fp32 unit roundoff
TINY = 2.0 ** -126             # smallest normal fp32: v_exp_f32 flushes what lies below
GUARD = 4096                   # guard elements on either side of an output (as kernel_check.GUARD)
QT_M, QT_N, QT_K = 64, 128, 64     # vectors per workgroup, codes per tile, dims per ring step (quantize.hip)

# ------------------------------------------------------------------------------------------------ measured constants
# Both are measured against the REFERENCE arithmetic on the CPU, never against the kernel (measure_chain / measure_kappa below;
# tests/test_quantiser_check.py re-measures and compares).  The kernel's own observed ratios are printed by the GPU tests under -s.
#
# CHAIN_MEASURED[dim]: the largest err / (u n S) that a plain sequential fp32 chain of the expanded form (chain_distances) reaches
# against fp64 over the inputs of DIST_CASES of that dim.  C_CHAIN = 4 x that (the margin covers the chain's order differing from the
# kernel's: four partial sums for the norms, fmaf instead of multiply-then-add).
CHAIN_MEASURED = {64: 0.0747, 128: 0.0484, 192: 0.0311, 256: 0.0298}      # (dim 64: set by the 40000 x 129 matrix)
C_CHAIN = {dim: 4.0 * v for dim, v in CHAIN_MEASURED.items()}
# (observed on MI355X, for information only: the kernel's max err / (u n S) over the same inputs is 0.0502 / 0.0205 / 0.0121 / 0.0106
# at dim 64 / 128 / 192 / 256 -- tests/test_gpu_quantiser.py prints it under -s)
#
# KAPPA_MEASURED[dim]: the largest relative error (beyond the 2^-126 flush) that a plain fp32 softmax of the fp64 logits -d64 / temp
# reaches against the fp64 softmax over the rows of SOFT_CASES of that dim.  KAPPA = 4 x that: covers rq_fast_exp2 (v_exp_f32) and
# the fp32 row sum of rq_softmax_rows_kernel.
KAPPA_MEASURED = {64: 4.37e-6, 128: 4.49e-6, 192: 3.87e-6, 256: 3.99e-6}
KAPPA = {dim: 4.0 * v for dim, v in KAPPA_MEASURED.items()}

# largest observed ratios (filled by the checks, printed by the GPU tests)
OBSERVED = {}


def _note(key, ratio):
    if key is not None and ratio == ratio:
        OBSERVED[key] = max(OBSERVED.get(key, 0.0), ratio)
    return ratio


# ------------------------------------------------------------------------------------------------ cases
# ks: codebook size per depth (equal sizes share ONE codebook tensor); kind: 'gauss' (N(0, 1) inputs and codebooks), 'resid'
# (a codeword + 0.05 x noise: depths >= 1 search with a small |r| against a large |c|), 'ties' (codebook rows hi copy rows lo,
# inputs are those rows + small noise), 'same' (every codebook row identical).  split: the launch form rqamd_rq_quantize picks.
Case = collections.namedtuple('Case', 'name dim ks n_vec kind split ties', defaults=('gauss', False, ()))

SINGLE_CASES = [
    # dim 64: one ring step per tile
    Case('d64_k1', 64, (1, 1), 5),                            # nstep 1; the norm DMA reads the codebook (K < 4)
    Case('d64_k2_3_5', 64, (2, 3, 5), 63),                    # nstep 1; K < 4 and the clamped norm chunk
    Case('d64_k127_ragged', 64, (127,), 64),                        # nstep 1, ragged
    Case('d64_k128', 64, (128, 128), 65),                     # nstep 1, full tile
    Case('d64_k129', 64, (129,), 130),                        # nstep 2; a last tile of one code
    Case('d64_k256', 64, (256,), 1),                          # nstep 2
    Case('d64_k257', 64, (257,), 63),                         # nstep 3
    Case('d64_k384', 64, (384,), 65),                         # nstep 3
    Case('d64_k500x4', 64, (500,) * 4, 130),                  # nstep 4, four depths
    # dim 128
    Case('d128_k64', 128, (64,), 1),                          # nstep 2
    Case('d128_k129', 128, (129,), 64),                       # nstep 4
    Case('d128_unshared', 128, (130, 70, 257), 130),          # nstep 4 / 2 / 6
    # dim 192 (NCH = 3)
    Case('d192_k128', 192, (128,), 63),                       # nstep 3
    Case('d192_k129', 192, (129,), 65),                       # nstep 6
    Case('d192_unshared', 192, (200, 129, 5), 130),           # nstep 6 / 6 / 3
    # dim 256
    Case('d256_k100', 256, (100,), 64),                       # nstep 4
    Case('d256_unshared', 256, (385, 128, 3), 130),           # nstep 16 / 4 / 4
    # residual-like inputs
    Case('d192_resid', 192, (300,) * 3, 130, 'resid'),
    Case('d256_resid', 256, (300,) * 3, 65, 'resid'),
]

SPLIT_CASES = [
    Case('s64_k1024', 64, (1024, 1024), 1, split=True),
    Case('s64_k1025_94tiles', 64, (1025, 1025), 6016, split=True),          # 5 splits, the last holds one ragged tile of one code
    Case('s64_unshared', 64, (1100, 1100, 1300), 70, split=True),           # n_split recomputed per depth
    Case('s64_k8190_cap', 64, (8190,), 5, split=True),                      # the 64-split cap, ragged last tile
    Case('s128_k1153', 128, (1153, 1153), 70, split=True),
    Case('s128_k2304', 128, (2304,), 1, split=True),
    Case('s192_k2304', 192, (2304, 2304), 70, split=True),
    Case('s192_k1153_94tiles', 192, (1153,), 6016, split=True),
    Case('s256_k1025', 256, (1025,) * 3, 70, split=True),
    Case('s256_k1024_94tiles', 256, (1024,), 6016, split=True),
    Case('s256_resid', 256, (1153,) * 3, 70, 'resid', split=True),
]

# copies at index distance 1 (neighbouring lane), 32 (next code group), 128 (next tile, same split), tiles_per_split * 128 (next
# split) and row K - 1 of a ragged tile copying row 0.  K = 2305 with 40 vector tiles: S = 12, two tiles per split, ten splits, the last
# of one code.  Under dbg_set_row_scale(96) the same case takes the single launch.
TIE_CASES = [
    Case('ties_split', 64, (2305, 2305), 2500, 'ties', True, ((5, 6), (40, 72), (260, 388), (300, 556), (0, 2304))),
    Case('ties_single', 128, (257, 257), 70, 'ties', False, ((5, 6), (40, 72), (100, 228), (0, 256))),
    Case('same_single', 64, (257, 257), 65, 'same'),
    Case('same_split', 64, (1100, 1100), 70, 'same', True),
]

# rq_distances / rq_soft_codes: one ragged single-tile and one split case per dim (neither call gates the split on K >= 1024), and
# rq_distances at 625 workgroups with S clamped to 1
DIST_CASES = [Case(f'dist{dim}_k77', dim, (77,), 65) for dim in (64, 128, 192, 256)] + \
             [Case(f'dist{dim}_k1153', dim, (1153,), 70, split=True) for dim in (64, 128, 192, 256)] + \
             [Case('dist64_wide', 64, (129,), 40000)]
SOFT_CASES = [Case(f'soft{dim}_k77', dim, (77, 77), 65) for dim in (64, 128, 192, 256)] + \
             [Case(f'soft{dim}_k1153', dim, (1153, 1153), 70, split=True) for dim in (64, 128, 192, 256)]

# the emulator's subset (fibers: small enough to run in both RQ_EMU_DMA modes): every dim, nstep 1 - 3, K < 4, one split case, the ties
EMU_CASES = [
    Case('emu64_k2_3_5', 64, (2, 3, 5), 9),                   # nstep 1, K < 4
    Case('emu64_k1', 64, (1, 1), 3),
    Case('emu64_k129', 64, (129,), 65),                       # nstep 2
    Case('emu64_k257', 64, (257,), 5),                        # nstep 3
    Case('emu128_k64', 128, (64, 64), 63),                    # nstep 2
    Case('emu192_k128', 192, (128,), 5),                      # nstep 3
    Case('emu192_k5', 192, (129, 5), 3),                      # nstep 6 / 3
    Case('emu256_k100', 256, (100,), 5),                      # nstep 4
    Case('emu64_split', 64, (1025, 1025), 5, split=True),     # 9 splits, the last holds one ragged tile of one code
]
EMU_TIE_CASES = [
    Case('emu_ties_single', 64, (257, 257), 8, 'ties', False, ((5, 6), (40, 72), (100, 228), (0, 256))),
    Case('emu_ties_split', 64, (1153, 1153), 10, 'ties', True, ((5, 6), (40, 72), (260, 388), (0, 1152))),      # one tile per split
    Case('emu_same', 64, (130, 130), 5, 'same'),
]


def soft_temp(dim):
    """temperature of the soft-code cases: the logits -d / temp then span a few tens, inside the fp32 exponent range"""
    return dim / 16.0


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def make_case(case):
    """(x (n_vec, dim), [codebook per depth]) of a case as fp32 numpy arrays from a generator seeded by the case's name; depths of equal
    K share one array (the same object)"""
    rng = np.random.default_rng(_seed(case.name))
    by_k = {}
    for K in case.ks:
        if K not in by_k:
            if case.kind == 'same':
                by_k[K] = np.tile(rng.standard_normal((1, case.dim), dtype=np.float32), (K, 1))
            else:
                by_k[K] = rng.standard_normal((K, case.dim), dtype=np.float32)
                for lo, hi in case.ties:
                    by_k[K][hi] = by_k[K][lo]
    cbs = [by_k[K] for K in case.ks]
    x = rng.standard_normal((case.n_vec, case.dim), dtype=np.float32)
    if case.kind == 'resid':
        x = (cbs[0][rng.integers(0, case.ks[0], case.n_vec)] + np.float32(0.05) * x).astype(np.float32)
    if case.kind == 'ties':
        lo = np.array([p[0] for p in case.ties])[np.arange(case.n_vec) % len(case.ties)]
        x = (cbs[0][lo] + np.float32(1e-3) * x).astype(np.float32)
    return x, cbs


def tie_targets(case):
    """depth-0 code of every input of a 'ties' case: the lower index of the pair its row was built from"""
    return np.array([p[0] for p in case.ties])[np.arange(case.n_vec) % len(case.ties)]


def nstep(K, dim):
    """ring steps of the single launch over one codebook: ceil(K / 128) tiles x dim / 64 chunks"""
    return -(-K // QT_N) * (dim // QT_K)


def split_plan(n_vec, ks, row_scale=1):
    """the launch form rqamd_rq_quantize picks (given a workspace): None for the single launch, else [(tiles_per_split, n_split)] per depth"""
    ntiles = -(-n_vec // QT_M)
    kmin = min(ks)
    if not (ntiles * row_scale < 96 and kmin >= 1024):
        return None
    S = min(512 // ntiles, 64, -(-kmin // QT_N))
    if S < 2:
        return None
    plan = []
    for K in ks:
        tk = -(-K // QT_N)
        tps = -(-tk // S)
        plan.append((tps, -(-tk // tps)))
    return plan


# ------------------------------------------------------------------------------------------------ references
def dist_ref(r, cb):
    """fp64 d64 = |r|^2 + |c|^2 - 2 r.c and S = |r|^2 + |c|^2 + 2 |r|.|c| of fp32 r (n, dim), cb (K, dim): two (n, K) matrices"""
    r64, c64 = r.double(), cb.double()
    base = (r64 * r64).sum(1)[:, None] + (c64 * c64).sum(1)[None]
    return base - 2.0 * (r64 @ c64.T), base + 2.0 * (r64.abs() @ c64.abs().T)


def err_bound(S, dim, c=1.0):
    """E = c u n S, n = dim + 4"""
    return (c * U * (dim + 4)) * S


def check_range(codes, ks, what=''):
    """no code < 0 or >= K (checked before anything indexes a codebook with them)"""
    for d, K in enumerate(ks):
        col = codes[:, d]
        bad = (col < 0) | (col >= K)
        if bool(bad.any()):
            i = int(bad.nonzero()[0, 0])
            raise AssertionError(f'{what}: {int(bad.sum())} codes of depth {d} outside [0, {K}); first: vector {i}, code {int(col[i])}')


def forced_residuals(x, cbs, codes):
    """yields (depth, residual) teacher-forced on `codes`: elementwise fp32 subtractions in depth order, the kernel's own operations"""
    r = x.clone()
    for d, cb in enumerate(cbs):
        yield d, r
        r = r - cb[codes[:, d]]


def reference_codes(x, cbs):
    """the fp64 argmin path from the reference alone (fp32 residual updates, as every implementation forms them)"""
    r, out = x.clone(), []
    for cb in cbs:
        k = dist_ref(r, cb)[0].argmin(1)
        out.append(k)
        r = r - cb[k]
    return torch.stack(out, 1)


def check_codes(x, cbs, codes, what='', key=None):
    """check 1: d64[k] - E[k] <= min_j (d64[j] + E[j]) with c = 1 for every vector and depth.  Returns the largest share of the allowance
    used, (d64[k] - min d64) / (E[k] + E[argmin]) (0 when every code is the fp64 argmin)."""
    dim = x.shape[1]
    check_range(codes, [cb.shape[0] for cb in cbs], what)
    used = 0.0
    for d, r in forced_residuals(x, cbs, codes):
        d64, S = dist_ref(r, cbs[d])
        E = err_bound(S, dim)
        k = codes[:, d:d + 1]
        lhs = (d64 - E).gather(1, k)[:, 0]
        rhs = (d64 + E).min(1).values
        bad = ~(lhs <= rhs)
        if bool(bad.any()):
            i = int(bad.nonzero()[0, 0])
            j = int(d64[i].argmin())
            raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} codes of depth {d} fail the certificate; first: vector {i}, code '
                                 f'{int(k[i, 0])} at d64 {float(d64[i, k[i, 0]])!r} (E {float(E[i, k[i, 0]]):.3e}) against code {j} at '
                                 f'{float(d64[i, j])!r} (E {float(E[i, j]):.3e})')
        dmin, jmin = d64.min(1)
        allow = E.gather(1, k)[:, 0] + E.gather(1, jmin[:, None])[:, 0]
        used = max(used, float(((d64.gather(1, k)[:, 0] - dmin) / allow.clamp_min(1e-300)).max()))
    return _note(key, used)


def ambiguous_share(x, cbs, codes=None):
    """check 2: the share of (vector, depth) pairs in which at least two codes satisfy the certificate inequality, from the fp64
    reference alone (codes None: along the reference's own argmin path; else along the given path)"""
    dim = x.shape[1]
    if codes is None:
        codes = reference_codes(x, cbs)
    n_amb, total = 0, 0
    for d, r in forced_residuals(x, cbs, codes):
        d64, S = dist_ref(r, cbs[d])
        E = err_bound(S, dim)
        passing = ((d64 - E) <= (d64 + E).min(1).values[:, None]).sum(1)
        n_amb += int((passing >= 2).sum())
        total += passing.numel()
    return n_amb / total


def first_equal_row(cb):
    """for every row of a codebook the lowest index of a row bit-equal to it (numpy int64 array)"""
    a = np.ascontiguousarray(cb.detach().cpu().numpy())
    v = a.view(np.dtype((np.void, a.shape[1] * a.itemsize)))[:, 0]
    _, first, inv = np.unique(v, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(np.int64)


def check_ties(cbs, codes, what=''):
    """check 3: every code is the lowest index among the codebook rows bit-equal to the chosen one (their kernel distances are
    bit-equal: same xn, same cn, same MFMA chain)"""
    check_range(codes, [cb.shape[0] for cb in cbs], what)
    got = codes.detach().cpu().numpy()
    for d, cb in enumerate(cbs):
        want = first_equal_row(cb)[got[:, d]]
        bad = got[:, d] != want
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise AssertionError(f'{what}: {int(bad.sum())} codes of depth {d} are not the lowest index of their duplicates; first: vector '
                                 f'{i}, code {int(got[i, d])}, lowest equal row {int(want[i])}')


def quants_ref(cbs, codes):
    """(depth, n_vec, dim): the depth-ordered fp32 sum of c[code], a sequential loop"""
    out, acc = [], None
    for d, cb in enumerate(cbs):
        e = cb[codes[:, d]]
        acc = e.clone() if acc is None else acc + e
        out.append(acc)
    return torch.stack(out)


def _bits_equal(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def check_quants(quants, cbs, codes, what=''):
    """check 4: quant_cum equals quants_ref bit for bit"""
    check_range(codes, [cb.shape[0] for cb in cbs], what)
    want = quants_ref(cbs, codes)
    if not _bits_equal(quants, want):
        bad = (quants.contiguous().view(torch.int32) != want.view(torch.int32)) if quants.shape == want.shape else None
        where = tuple(bad.nonzero()[0].tolist()) if bad is not None else 'shape'
        raise AssertionError(f'{what}: quant_cum differs from the depth-ordered fp32 sum of c[code]; first at {where}')


def check_embed(embed, mode, cbs, codes, what=''):
    """check 4, rq_embed: mode 0 (n_vec, dim) the sum over depth, 1 (n_vec, depth, dim) c[code], 2 (n_vec, depth, dim) the depth-cumsum"""
    if mode == 1:
        want = torch.stack([cb[codes[:, d]] for d, cb in enumerate(cbs)], 1)
    else:
        q = quants_ref(cbs, codes)
        want = q[-1] if mode == 0 else q.permute(1, 0, 2).contiguous()
    if not _bits_equal(embed, want):
        raise AssertionError(f'{what}: rq_embed mode {mode} differs from the depth-ordered fp32 sum')


def check_distances(dist, x, cb, c, what='', key=None, ref=None):
    """check 5: |dist - d64| <= c u n S elementwise.  Returns the observed max err / (u n S)."""
    d64, S = ref if ref is not None else dist_ref(x, cb)
    unit = err_bound(S, x.shape[1])
    err = (dist.double() - d64).abs()
    bad = ~(err <= c * unit)                      # NaN counts as bad
    ratio = float((err / unit.clamp_min(1e-300)).max())
    if bool(bad.any()):
        t = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} distances outside c = {c:.4g}; first at {t}: {float(dist[t])!r}, d64 '
                             f'{float(d64[t])!r}, |err| {float(err[t]):.3e} > {float(c * unit[t]):.3e}; largest err / (u n S) {ratio:.4f}')
    return _note(key, ratio)


def chain_distances(x, cb):
    """a plain sequential fp32 chain of the expanded form on the CPU (numpy, multiply then add, dims in order): xn + cn - 2 acc"""
    x, cb = np.asarray(x, np.float32), np.asarray(cb, np.float32)
    two = np.float32(2.0)
    acc = np.zeros((x.shape[0], cb.shape[0]), np.float32)
    xn, cn = np.zeros(x.shape[0], np.float32), np.zeros(cb.shape[0], np.float32)
    for i in range(x.shape[1]):
        acc += x[:, i:i + 1] * cb[None, :, i]
        xn += x[:, i] * x[:, i]
        cn += cb[:, i] * cb[:, i]
    return (xn[:, None] + cn[None]) - two * acc


def measure_chain(cases=None):
    """{dim: the largest err / (u n S) of chain_distances against fp64 over the depth-0 inputs of the cases of that dim}"""
    out = {}
    for case in (DIST_CASES if cases is None else cases):
        x, cbs = make_case(case)
        d64, S = dist_ref(torch.from_numpy(x), torch.from_numpy(cbs[0]))
        err = (torch.from_numpy(chain_distances(x, cbs[0])).double() - d64).abs()
        out[case.dim] = max(out.get(case.dim, 0.0), float((err / err_bound(S, case.dim)).max()))
    return out


def soft_ref(d64, temp):
    """fp64 softmax of -d64 / temp over the codebook"""
    z = -d64 / temp
    e = torch.exp(z - z.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def soft_fp32(d64, temp):
    """a plain fp32 softmax of the fp64 logits -d64 / temp (rounded to fp32 first)"""
    z = (-d64 / temp).float()
    e = torch.exp(z - z.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def measure_kappa(cases=None):
    """{dim: the largest (|p32 - p64| - 2^-126) / p64 of soft_fp32 against soft_ref over every row and depth (the reference's own code
    path) of the cases of that dim}"""
    out = {}
    for case in (SOFT_CASES if cases is None else cases):
        x, cbs = make_case(case)
        x, cbs = torch.from_numpy(x), [torch.from_numpy(c) for c in cbs]
        temp = soft_temp(case.dim)
        for d, r in forced_residuals(x, cbs, reference_codes(x, cbs)):
            d64, _ = dist_ref(r, cbs[d])
            p64 = soft_ref(d64, temp)
            rel = ((soft_fp32(d64, temp).double() - p64).abs() - TINY).clamp_min(0.0) / p64.clamp_min(1e-300)
            out[case.dim] = max(out.get(case.dim, 0.0), float(rel.max()))
    return out


def check_soft(soft, x, cbs, codes, temp, kappa, what='', key=None):
    """check 6: soft (n_vec, depth, K) against the fp64 softmax along the teacher-forced path, and every row sums to 1 within K u.
    Returns the largest share of the bound used, max |soft - p64| / bound."""
    dim = x.shape[1]
    check_range(codes, [cb.shape[0] for cb in cbs], what)
    seen = 0.0
    for d, r in forced_residuals(x, cbs, codes):
        K = cbs[d].shape[0]
        d64, S = dist_ref(r, cbs[d])
        p64 = soft_ref(d64, temp)
        grow = torch.expm1(2.0 * err_bound(S, dim).max(1, keepdim=True).values / temp)
        got = soft[:, d].double()
        err = (got - p64).abs()
        bound = p64 * (grow + kappa) + TINY
        bad = ~(err <= bound)
        seen = max(seen, float((err / bound).max()))
        if bool(bad.any()):
            t = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} soft codes of depth {d} outside the bound; first at {t}: '
                                 f'{float(got[t])!r}, p64 {float(p64[t])!r}, |err| {float(err[t]):.3e} > {float(bound[t]):.3e}')
        off = (got.sum(1) - 1.0).abs()
        if not bool((off <= K * U).all()):
            raise AssertionError(f'{what}: a soft-code row of depth {d} sums to 1 +- {float(off.max()):.3e} > K u = {K * U:.3e}')
    return _note(key, seen)


def check_norms(cn, cb, what=''):
    """check 7: |cn - cn64| <= (dim / 4 + 2) u cn64"""
    cn64 = (cb.double() ** 2).sum(1)
    err = (cn.double() - cn64).abs()
    bad = ~(err <= (cb.shape[1] / 4 + 2) * U * cn64)
    if bool(bad.any()):
        i = int(bad.nonzero()[0, 0])
        raise AssertionError(f'{what}: {int(bad.sum())} code norms outside the bound; first: code {i}, {float(cn[i])!r} against {float(cn64[i])!r}')


# ------------------------------------------------------------------------------------------------ buffers
def guarded_codes(shape, device):
    """an int64 output of `shape` inside a flat buffer with GUARD elements on either side, everything -1: (buf, view)"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), -1, dtype=torch.int64, device=device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def check_code_guard(buf, n, what=''):
    """everything of buf outside [GUARD, GUARD + n) is still -1"""
    for part, name in ((buf[:GUARD], 'before'), (buf[GUARD + n:], 'after')):
        bad = part != -1
        if bool(bad.any()):
            raise AssertionError(f'{what}: {int(bad.sum())} stores {name} the codes (first at guard offset {int(bad.nonzero()[0, 0])})')


# ------------------------------------------------------------------------------------------------ one case through a binding
def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


def device_case(case, dev):
    """(x, [codebook per depth]) of a case on `dev`, each the front view of a NaN-filled buffer; shared codebooks stay one tensor"""
    x, cbs = make_case(case)
    moved = {}
    for c in cbs:
        if id(c) not in moved:
            moved[id(c)] = kc.poisoned(torch.from_numpy(c).to(dev), 37)
    return kc.poisoned(torch.from_numpy(x).to(dev)), [moved[id(c)] for c in cbs]


def checked_norms(nat, cbs, what=''):
    """rq_code_norms of every codebook (check 7), each the front view of a NaN-filled buffer"""
    done = {}
    for cb in cbs:
        if cb.data_ptr() not in done:
            cn = nat.rq_code_norms(cb)
            check_norms(cn, cb, what)
            done[cb.data_ptr()] = kc.poisoned(cn, 5)
    return [done[cb.data_ptr()] for cb in cbs]


def launch_quantize(nat, x, cbs, norms, what=''):
    """rq_quantize into guard-filled outputs (check 8): (codes, quant_cum)"""
    (n_vec, dim), depth = x.shape, len(cbs)
    cbuf, codes = guarded_codes((n_vec, depth), x.device)
    qbuf, quants = kc.guarded((depth, n_vec, dim), torch.float32, x.device)
    nat.rq_quantize(x, cbs, norms=norms, out=(codes, quants))
    _sync(x.device)
    check_code_guard(cbuf, codes.numel(), what)
    kc.check_guard(qbuf, quants.numel(), what)
    return codes, quants


def run_quantize_case(nat, case, dev, other_form=False):
    """one case of the lists above through nat.rq_quantize / rq_embed with every check that applies; other_form: once more under
    dbg_set_row_scale(96) (the single launch over the same vectors), codes and quants bit-identical.  Returns the share of the
    certificate's allowance that the codes used."""
    x, cbs = device_case(case, dev)
    norms = checked_norms(nat, cbs, case.name)
    codes, quants = launch_quantize(nat, x, cbs, norms, case.name)
    used = check_codes(x, cbs, codes, case.name, key='certificate')
    check_ties(cbs, codes, case.name)
    check_quants(quants, cbs, codes, case.name)
    for mode in (0, 1, 2):
        check_embed(nat.rq_embed(codes, cbs, mode), mode, cbs, codes, case.name)
    if case.kind == 'ties':
        assert np.array_equal(codes[:, 0].cpu().numpy(), tie_targets(case)), f'{case.name}: a duplicated row did not go to its lowest index'
    elif case.kind == 'same':
        assert int(codes.abs().max()) == 0, f'{case.name}: identical codebook rows, yet a code != 0'
    else:
        share = ambiguous_share(x, cbs, codes)
        assert share <= 0.01, f'{case.name}: the certificate leaves {share:.2%} of the (vector, depth) pairs open'
    codes_only, none = nat.rq_quantize(x, cbs, want_quants=False, norms=norms)
    assert none is None and torch.equal(codes_only, codes), f'{case.name}: codes differ without quant_cum'
    if other_form:
        nat.dbg_set_row_scale(96)
        try:
            codes_b, quants_b = launch_quantize(nat, x, cbs, norms, case.name + ' (single launch)')
        finally:
            nat.dbg_set_row_scale(1)
        assert torch.equal(codes_b, codes), f'{case.name}: the two launch forms disagree on {int((codes_b != codes).sum())} codes'
        assert _bits_equal(quants_b, quants), f'{case.name}: the two launch forms disagree on quant_cum'
    return used


def run_distance_case(nat, case, dev):
    """rq_distances of a case's inputs and first codebook into a guarded output: check 5 with c = 1 and with C_CHAIN; launched twice
    (same bits).  Returns the observed max err / (u n S)."""
    x, cbs = device_case(case, dev)
    cb = cbs[0]
    cn = checked_norms(nat, [cb], case.name)[0]
    buf, out = kc.guarded((case.n_vec, cb.shape[0]), torch.float32, dev)
    nat.rq_distances(x, cb, cn, out=out)
    _sync(dev)
    kc.check_guard(buf, out.numel(), case.name)
    ref = dist_ref(x, cb)
    ratio = check_distances(out, x, cb, 1.0, case.name, ref=ref)
    check_distances(out, x, cb, C_CHAIN[case.dim], case.name, key=f'distances dim {case.dim}', ref=ref)
    again = nat.rq_distances(x, cb, cn)
    assert _bits_equal(again, out), f'{case.name}: two launches, different distances'
    return ratio


def run_soft_case(nat, case, dev):
    """rq_soft_codes (deterministic) of a case into guarded outputs: the codes under checks 1 - 3 and equal to rq_quantize's, the soft
    codes under check 6; then the stochastic form: every drawn code has positive soft mass.  Returns the largest share of the soft
    codes' bound used."""
    x, cbs = device_case(case, dev)
    norms = checked_norms(nat, cbs, case.name)
    temp, K, depth = soft_temp(case.dim), case.ks[0], len(case.ks)
    sbuf, soft = kc.guarded((case.n_vec, depth, K), torch.float32, dev)
    cbuf, codes = guarded_codes((case.n_vec, depth), dev)
    nat.rq_soft_codes(x, cbs, norms, temp=temp, out=(soft, codes))
    _sync(dev)
    kc.check_guard(sbuf, soft.numel(), case.name)
    check_code_guard(cbuf, codes.numel(), case.name)
    check_codes(x, cbs, codes, case.name, key='certificate')
    check_ties(cbs, codes, case.name)
    share = ambiguous_share(x, cbs, codes)
    assert share <= 0.01, f'{case.name}: the certificate leaves {share:.2%} of the (vector, depth) pairs open'
    qcodes, _ = nat.rq_quantize(x, cbs, want_quants=False, norms=norms)
    assert torch.equal(qcodes, codes), f'{case.name}: rq_soft_codes and rq_quantize disagree on the codes'
    seen = check_soft(soft, x, cbs, codes, temp, KAPPA[case.dim], case.name, key=f'soft codes dim {case.dim}')
    s1, c1 = nat.rq_soft_codes(x, cbs, norms, temp=temp, stochastic=True, seed=3, offset=0)
    _sync(dev)
    check_range(c1, case.ks, case.name + ' (stochastic)')
    assert float(torch.gather(s1, 2, c1.unsqueeze(-1)).min()) > 0.0, f'{case.name}: a drawn code without soft mass'
    return seen
