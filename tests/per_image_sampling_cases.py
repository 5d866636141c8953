"""Shared by tests/test_emu_per_image_sampling.py (host emulator) and tests/test_gpu_per_image_sampling.py (MI355X): the checks of
per-image sampling parameters and seeds -- rqamd_sample_logits_rows, rqamd_rqt_sample_rows, and the tensor arguments of
RQTransformer.sample / sample_guided with RQTransformer.seeds().  Models, conditionings and seeds come from
tests/masked_sampling_cases.py.  Apart from the comparison with the oracle every comparison is exact, and the yardstick is always an
entry point that takes one value per call: row r of a per-row call is what the scalar call with r's values gives for row r."""
import ctypes

import numpy as np
import torch

import oracle
import guided_sampling_cases as G
import masked_sampling_cases as M

SMP_CAP = 2048                    # csrc/rqt_kernels.hip: more keys than this tied into the top k -> the register kernel hands the row back
VOCABS = (16384, 500, 499, 7)     # register kernel with rows past SMP_CAP; register kernel; V % 4 != 0: none; smaller than every k


# ------------------------------------------------------------------------------------------------ 1. kernel: rows against scalars
def kernel_table(V):
    """12 rows of (temperature, top_k or None, top_p or None), the classes interleaved: unfiltered (streaming kernel when no
    probabilities are asked for), 0 < k < V (register kernel where V allows it), everything else (general kernel); rows 9 .. 11 are
    the hard logits rows of kernel_logits"""
    return [(1.0, None, None), (1.0, 10, None), (1.0, 10, 0.9), (0.7, None, None), (0.8, 10, None), (1.0, None, 0.7),
            (1.0, 1, None), (1.0, V, None), (1.0, None, 1.0), (1.0, 10, None), (1.0, 10, None), (0.8, 10, 0.9)]


HANDBACK_ROWS = (9, 10)           # two-valued row (V > SMP_CAP only) and NaN row: the register kernel gives them to the general kernel


def kernel_logits(V, seed):
    """N(0, 2) rows; row 9: two distinct values, 60 % at the upper one (more than SMP_CAP keys tie into the top 10 at V = 16384);
    row 10: min(12, V - 2) NaNs, so the 10th largest key is NaN wherever top-k 10 is in effect; row 11: constant"""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((12, V))).astype(np.float32)
    x[9] = rng.choice([0.5, 1.5], V, p=[0.4, 0.6]).astype(np.float32)
    x[10, rng.choice(V, min(12, V - 2), replace=False)] = np.nan
    x[11] = 0.25
    return x


def table_tensors(table, device):
    T = torch.tensor([t for t, _, _ in table], dtype=torch.float32, device=device)
    K = torch.tensor([0 if k is None else k for _, k, _ in table], dtype=torch.int32, device=device)
    P = torch.tensor([-1.0 if p is None else p for _, _, p in table], dtype=torch.float32, device=device)
    return T, K, P


def _same_probs(a, b):
    """bit-equal, NaN included (a row the sampler could not normalise is the same garbage in both)"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def scalar_row_flags(nat, logits, t, k, p, seed, offset):
    """row_flags after rqamd_sample_logits (the binding's sample_logits keeps them to itself)"""
    rows, V = logits.shape
    flags = torch.zeros((rows,), dtype=torch.int32, device=logits.device)
    out = torch.empty((rows,), dtype=torch.int64, device=logits.device)
    with nat.on_device_of(logits):
        nat.check(nat.lib().rqamd_sample_logits(nat.ptr(logits), rows, V, float(t), 0 if k is None else int(k), -1.0 if p is None else float(p),
                                                seed, offset, nat.ptr(out), None, nat.ptr(flags), nat.stream_of(logits)))
    return flags


def check_rows_against_scalar(nat, V, device, want_probs, seed=11, offset=8):
    """samples (and probs_out) of row r of sample_logits_rows == row r of sample_logits(logits, T_r, k_r, p_r, seed, offset) over the
    same matrix.  want_probs = False lets the unfiltered rows take the streaming kernel, True holds the probabilities as well."""
    table = kernel_table(V)
    logits = torch.from_numpy(kernel_logits(V, V)).to(device)
    T, K, P = table_tensors(table, device)
    got, gprobs = nat.sample_logits_rows(logits, T, K, P, seed=seed, offset=offset, want_probs=want_probs)
    assert got.shape == (12,) and got.dtype == torch.int64 and bool(((got >= 0) & (got < V)).all())
    done = {}
    for r, (t, k, p) in enumerate(table):
        if (t, k, p) not in done:
            done[(t, k, p)] = nat.sample_logits(logits, t, k, p, seed=seed, offset=offset, want_probs=want_probs)
        want, wprobs = done[(t, k, p)]
        assert int(got[r]) == int(want[r]), (V, r, table[r], int(got[r]), int(want[r]))
        if want_probs:
            assert _same_probs(gprobs[r], wprobs[r]), (V, r, table[r])
    if V <= 16384 and V % 4 == 0 and V > 10:
        # the hand-back rows do take the hand-back in the scalar call (and, the results being equal, in the per-row call)
        flags = scalar_row_flags(nat, logits, 1.0, 10, None, seed, offset).cpu()
        assert int(flags[10]) != 0, 'the NaN row was not handed to the general kernel'
        if V > SMP_CAP:
            assert int(flags[9]) != 0, 'the two-valued row was not handed to the general kernel'
        assert int(flags[1]) == 0
    return got


def check_row_seeds(nat, V, device):
    """with seeds, row r == row 0 of sample_logits(logits[r:r+1], T_r, k_r, p_r, seed=seeds[r], offset=0), wherever r stands"""
    table = kernel_table(V)
    logits = torch.from_numpy(kernel_logits(V, V)).to(device)
    T, K, P = table_tensors(table, device)
    seeds = [3, 2 ** 40 + 5, 3, 0, 7, 2 ** 62, 1, 9, 11, 13, 15, 17]
    got, _ = nat.sample_logits_rows(logits, T, K, P, seeds=torch.tensor(seeds, dtype=torch.int64, device=device), seed=99, offset=0)
    for r, (t, k, p) in enumerate(table):
        want, _ = nat.sample_logits(logits[r:r + 1].contiguous(), t, k, p, seed=seeds[r], offset=0)
        assert int(got[r]) == int(want[0]), (V, r, table[r])
    # the place in the matrix does not matter: the rows reversed give the samples reversed
    rev = torch.arange(11, -1, -1, device=device)
    got_r, _ = nat.sample_logits_rows(logits[rev].contiguous(), T[rev].contiguous(), K[rev].contiguous(), P[rev].contiguous(),
                                      seeds=torch.tensor(seeds[::-1], dtype=torch.int64, device=device))
    assert torch.equal(got_r, got[rev])


# ------------------------------------------------------------------------------------------------ 2. kernel against the oracle
ORACLE_TABLE = [(1.0, None, None), (0.7, None, None), (1.0, 10, None), (0.8, 10, None), (1.0, 1, None), (1.0, 10, 0.9),
                (1.0, None, 0.7), (0.8, 50, 0.95)]


def check_rows_against_oracle(nat, device, V=500, seed=17):
    """probs_out of a mixed table against oracle.sampler.filtered_probs row by row, on tie-free rows, with the bounds of
    tests/test_emu_kernels.py::test_emu_sampler_filter: total variation below 1e-5 and equal support size"""
    x = (2.0 * np.random.default_rng(seed).standard_normal((len(ORACLE_TABLE), V))).astype(np.float32)
    T, K, P = table_tensors(ORACLE_TABLE, device)
    _, probs = nat.sample_logits_rows(torch.from_numpy(x).to(device), T, K, P, want_probs=True, want_samples=False)
    o = probs.cpu().numpy()
    for r, (t, k, p) in enumerate(ORACLE_TABLE):
        ref = oracle.filtered_probs(x[r:r + 1], t, k, p)[0]
        assert len(np.unique(x[r])) == V and len(np.unique(ref[ref > 0])) == int((ref > 0).sum()), f'row {r} is not tie-free'
        tv = 0.5 * float(np.abs(o[r] - ref).sum())
        print(f'row {r} {ORACLE_TABLE[r]}: total variation {tv:.3g}, support {int((o[r] > 0).sum())} / {int((ref > 0).sum())}')
        assert tv < 1e-5, (r, tv)
        assert int((o[r] > 0).sum()) == int((ref > 0).sum()), r


# ------------------------------------------------------------------------------------------------ 3. engine: heterogeneous == homogeneous
# three parameter groups, interleaved by row; group 0 is unfiltered (the streaming kernel next to the register and general kernels)
GROUPS = (dict(temperature=1.0, top_k=None, top_p=None), dict(temperature=0.8, top_k=50, top_p=0.9), dict(temperature=1.0, top_k=10, top_p=None))
SCALES = (1.0, 3.0, 0.5)


def group_of(B):
    return [b % len(GROUPS) for b in range(B)]


def group_tensors(B, V, device, per_depth=False, D=4):
    """the per-image arguments of the interleaved groups: temperature (B,), top_k (B,) int64 (None: V, which is "off") and top_p (B,)
    (None: 1.0); per_depth: top_k / top_p as (B, D)"""
    g = group_of(B)
    T = torch.tensor([GROUPS[i]['temperature'] for i in g], dtype=torch.float32, device=device)
    K = torch.tensor([V if GROUPS[i]['top_k'] is None else GROUPS[i]['top_k'] for i in g], dtype=torch.int64, device=device)
    P = torch.tensor([1.0 if GROUPS[i]['top_p'] is None else GROUPS[i]['top_p'] for i in g], dtype=torch.float32, device=device)
    if per_depth:
        K, P = K[:, None].expand(B, D).contiguous(), P[:, None].expand(B, D).contiguous()
    return dict(temperature=T, top_k=K, top_p=P)


def check_hetero(ar, aux, partial, cond, seed, uncond=None, per_depth=False, **extra):
    """The rows of group g in the per-image call equal those rows of the call that gives g's values to all rows, after the same
    manual_seed (the other rows draw other codes there, which must not matter).  uncond given: sample_guided, one scale per group."""
    B, dev = partial.shape[0], partial.device
    g = torch.tensor(group_of(B), device=dev)
    kw = group_tensors(B, max(ar.vocab_size), dev, per_depth, ar.block_size[2])
    fn = ar.sample
    if uncond is not None:
        fn = ar.sample_guided
        extra = dict(extra, uncond=uncond)
        kw['guidance_scale'] = torch.tensor([SCALES[i] for i in group_of(B)], dtype=torch.float32, device=dev)
    M.seed_all(seed)
    got = fn(partial, aux, cond=cond, **kw, **extra)
    assert got.shape == partial.shape and got.dtype == torch.int64
    outs = []
    for i, grp in enumerate(GROUPS):
        skw = dict(grp)
        if uncond is not None:
            skw['guidance_scale'] = SCALES[i]
        M.seed_all(seed)
        want = fn(partial, aux, cond=cond, **skw, **extra)
        assert torch.equal(got[g == i], want[g == i]), (f'rows of group {i} differ from the call made with its values', grp, sorted(extra))
        outs.append(want)
    return got, outs


# ------------------------------------------------------------------------------------------------ 4. seeds
def check_position_independent_logits(ar, aux, codes, cond, perm, amp=False):
    """the engine's logits of an image do not depend on its row at a fixed batch size (what checks 4a / 4b rest on)"""
    a = ar.teacher_forced_logits(codes, aux, cond=cond, amp=amp)
    b = ar.teacher_forced_logits(codes[perm].contiguous(), aux, cond=cond[perm].contiguous(), amp=amp)
    assert torch.equal(a.view(torch.int32)[perm], b.view(torch.int32)), 'engine finding: the logits of an image depend on its row'


def check_seed_permutation(ar, aux, partial, cond, seeds, perm, **extra):
    """(a) rows of partial_sample, cond, the parameter tensors and seeds permuted: the output is permuted the same way"""
    B, dev = partial.shape[0], partial.device
    kw = group_tensors(B, max(ar.vocab_size), dev)
    with ar.seeds(seeds):
        a = ar.sample(partial, aux, cond=cond, **kw, **extra)
    pl = perm.tolist()
    pkw = {k: v[perm].contiguous() for k, v in kw.items()}
    pextra = {k: (v[perm].contiguous() if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for k, v in extra.items()}
    with ar.seeds([seeds[i] for i in pl]):
        b = ar.sample(partial[perm].contiguous(), aux, cond=cond[perm].contiguous(), **pkw, **pextra)
    assert torch.equal(b, a[perm]), 'a seeded image depends on its place in the batch'
    return a


def check_seed_single_image(ar, aux, partial, cond, seeds, seeded_out, b, keep_mask, direct=False):
    """(b) image b of the seeded call == row 0 of torch.manual_seed(seeds[b]); sample(...) over the same B with the image at row 0 and
    its own values as the scalars.  direct (the emulator, whose CPU generator has no Philox offset to reset: sample() draws a random
    one there): the same call made at the engine's masked entry point with seed = seeds[b], offset = 0."""
    B = partial.shape[0]
    order = torch.tensor([b] + [i for i in range(B) if i != b], device=partial.device)
    xs, c, keep = partial[order].contiguous(), cond[order].contiguous(), keep_mask[order].contiguous()
    grp = GROUPS[group_of(B)[b]]
    if direct:
        tk, tp = ar._filter_lists(grp['top_k'], grp['top_p'])
        want = ar._eng(False).sample_masked(xs, keep.to(torch.uint8), None, c, ar._checked_codebooks(aux), grp['temperature'], tk, tp,
                                            seeds[b], 0, ar.use_graph)
    else:
        M.seed_all(seeds[b])
        want = ar.sample(xs, aux, cond=c, keep_mask=keep, **grp)
    assert torch.equal(seeded_out[b], want[0]), f'image {b} is not row 0 of the call seeded with its seed'


def check_seed_streams(ar, aux, partial, cond, state_fn, **extra):
    """(c) a seeded call leaves the generator alone; (d) equal inputs and equal seeds give equal images, unequal seeds other ones"""
    B = partial.shape[0]
    same_p = partial[:1].expand_as(partial).contiguous()
    same_c = cond[:1].expand_as(cond).contiguous()
    seeds = [5, 5] + [9 + i for i in range(B - 2)]
    before = state_fn()
    with ar.seeds(torch.tensor(seeds)):
        out = ar.sample(same_p, aux, cond=same_c, **extra)
    assert torch.equal(before, state_fn()), 'a seeded call consumed the generator'
    assert torch.equal(out[0], out[1])
    assert not torch.equal(out[0], out[2])
    return out


# ------------------------------------------------------------------------------------------------ 6. host loops
def three_code_mask(B, H=4, W=4, D=4):
    """keep everything but three codes (the uncached loop runs one teacher-forced pass of the whole map for each)"""
    keep = torch.ones((B, H, W, D), dtype=torch.bool)
    keep[0, 0, 3, 1] = False
    keep[:, 1, 2, :2] = False
    return keep


def check_torch_support(nat, ar, aux, out, cond, keep, amp=False):
    """sampler='torch' with per-image values: every drawn code lies inside its own row's top-k (the support check of
    guided_sampling_cases.py at s = 1, row by row with the row's k; unfiltered rows have nothing to check)"""
    B = out.shape[0]
    logits = ar.teacher_forced_logits(out, aux, cond=cond, amp=amp)
    for d, v in enumerate(ar.vocab_size):
        logits[..., d, v:] = float('-inf')
    mine = torch.gather(logits, -1, out[..., None])[..., 0]
    for b in range(B):
        k = GROUPS[group_of(B)[b]]['top_k']
        if k is None:
            continue
        bad = (~keep[b].to(out.device)) & ~(mine[b] >= M.kth_largest(logits[b], k))
        assert not bool(bad.any()), f'image {b}: {int(bad.sum())} drawn codes outside its top-{k}'


# ------------------------------------------------------------------------------------------------ 7. errors
def value_error_cases(B, D, V, device):
    """(name, keyword arguments of sample()) that must raise ValueError before anything is launched"""
    T = torch.ones(B, device=device)
    return [('temperature shape', dict(temperature=torch.ones(B + 1, device=device))),
            ('temperature 2-d', dict(temperature=torch.ones((B, D), device=device))),
            ('top_k shape', dict(top_k=torch.full((B, D + 1), 5, dtype=torch.int64, device=device))),
            ('top_p shape', dict(top_p=torch.full((B + 1,), 0.9, device=device))),
            ('top_k float', dict(top_k=torch.full((B,), 5.0, device=device))),
            ('temperature zero', dict(temperature=torch.tensor([1.0] * (B - 1) + [0.0], device=device))),
            ('temperature negative', dict(temperature=-T)),
            ('temperature nan', dict(temperature=T * float('nan'))),
            ('temperature inf', dict(temperature=T * float('inf')))]


def c_sample_rows(nat, ar, aux, partial, cond, temperature, top_k, top_p, scale=None, null=()):
    """rqamd_rqt_sample_rows called directly (everything kept, so nothing is drawn): the status code"""
    eng, cbs = ar._eng(False), ar._checked_codebooks(aux)
    B, D = partial.shape[0], partial.shape[-1]
    keep8 = torch.ones(partial.shape, dtype=torch.uint8, device=partial.device)
    out = torch.empty_like(partial)
    args = dict(T=(ctypes.c_float * B)(*temperature), k=(ctypes.c_int * (B * D))(*top_k), p=(ctypes.c_float * (B * D))(*top_p),
                s=None if scale is None else (ctypes.c_float * B)(*scale), partial=nat.ptr(partial), out=nat.ptr(out))
    for n in null:
        args[n] = None
    active = (ctypes.c_uint8 * 16)()
    return eng._L.rqamd_rqt_sample_rows(eng._h, args['partial'], nat.ptr(keep8), active, nat.ptr(cond), None, B, nat._ptr_array(cbs[:D]), 0, 0,
                                        args['T'], args['k'], args['p'], args['s'], None, 1, 0, 0, args['out'], None), eng._L.rqamd_last_error()
