"""The sampler kernels (csrc/rqt_kernels.hip: sample_gumbel_kernel, sample_topk_kernel + sample_tail, sample_kernel; scalar, guided and
per-row builds) certified on the MI355X against the exact Philox reference and fp64 filters of tests/sampler_check.py (the evidence
that those checks can fail is tests/test_sampler_check.py; the emulator twin is tests/test_emu_sampler.py).  Every draw of every row
is certified -- the filtered kernels on their own kept set by the fp64 exponential race, the streaming kernel by the fp64 Gumbel score
-- every kept set against the exact top-k set and the top-p certificate, every probability elementwise, and the hand-back flags of the
register kernel exactly.  Every filtered case runs with row_flags (register kernel where eligible) and without (general kernel), and
once more without probs_out (identical draws).  Cases: sampler_check.CASES (vocabulary forms 1 .. 36000, top-k 1 / V - 1 / V, SMP_CAP
and SMP_CAP + 1 survivors, 256 / 257 / 1024 keys in one bf16 bucket, negative-only, +-0.0 at the threshold, NaN and few-valued rows,
top-p 0 / 1e-8 / 0.5 / 0.95 / 1 - 2^-24 / 1, masks, T = 0.05 and 20), the stream cases (high words of seed and offset over 300 rows),
per-row tables and row seeds, a probe row that pins the word -> u mapping, V = 36001, and one sample() and one sample_guided() call of
the tiny model.  Run with -s for the observed maxima (copied to profiles/sampler_certificate.txt)."""
import numpy as np
import pytest
import torch

import kernel_check as kc
import sampler_check as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    yield _native
    for key in sorted(sc.OBSERVED):
        print(f'\nsampler: {key:24s} largest observed {sc.OBSERVED[key]:.4g}', end='')
    print(f'\nsampler: C_RACE {sc.C_RACE} u, C_GUMBEL {sc.C_GUMBEL} u, probability bound and top-p mass at c = 1')


def _run(nat, case):
    x = sc.build_logits(case)
    worst, near, flags = sc.run_scalar_case(nat, x, case.T, case.k, case.p, case.seed, case.offset, DEV, case.name)
    print(f'{case.name}: largest deficit {worst:.3g} u, rows with a runner-up inside the tolerance {near} of {case.rows}')
    return flags


@pytest.mark.parametrize('case', sc.CASES, ids=lambda c: c.name)
def test_sampler_case(nat, case):
    flags = _run(nat, case)
    if case.name.startswith('cap_'):
        # k = SMP_CAP distinct keys stay in the register kernel, k = SMP_CAP + 1 are handed to the general kernel
        assert (flags == int(case.k > sc.SMP_CAP)).all()


@pytest.mark.parametrize('case', sc.stream_cases(500), ids=lambda c: c.name)
def test_sampler_stream(nat, case):
    """high words of seed and offset, 300 rows: certified against the Philox reference, not against another call"""
    _run(nat, case)


def test_sampler_probe_row(nat):
    """the row whose draw depends on u at a word below 64 (sampler_check.PROBE): all three kernels"""
    x, seed, offset = sc.probe_logits()
    for k in (None, 2):
        sc.run_scalar_case(nat, x, 1.0, k, None, seed, offset, DEV, f'probe k={k}')


def test_sampler_vocab_36001_is_refused(nat):
    """one past the largest vocabulary: the unsupported status, and nothing written"""
    x = kc.poisoned(torch.zeros((8, sc.V_MAX + 1), dtype=torch.float32, device=DEV))
    for k, p in ((None, None), (10, 0.9)):
        for want_probs in (True, False):
            got = sc.call_scalar(nat, x, 1.0, k, p, 7, 5, want_probs=want_probs, expect=-2)
            assert got.status == -2 and got.samples is None and got.probs is None


@pytest.mark.parametrize('V', [16384, 500, 499, 7])
def test_sampler_rows(nat, V):
    """rqamd_sample_logits_rows: the mixed table of per_image_sampling_cases with the call's seed, then with one seed per row (row
    field 0, key seeds[r]): every row certified against the reference with its own values"""
    import per_image_sampling_cases as P
    x, table = P.kernel_logits(V, V), P.kernel_table(V)
    sc.run_rows_case(nat, x, table, None, 2 ** 32 + 9, 2 ** 40 + 3, DEV, f'rows V{V}')
    seeds = [3, 2 ** 40 + 5, 3, 0, 7, 2 ** 62, 1, 2 ** 63 + 11, 2 ** 32, 2 ** 32 - 1, 15, 17]
    sc.run_rows_case(nat, x, table, seeds, 99, 0, DEV, f'row seeds V{V}')
    sc.run_rows_case(nat, x, table, seeds, 99, 2 ** 32 + 1, DEV, f'row seeds V{V} with an offset')


# ------------------------------------------------------------------------------------------------ engine
ENGINE_TOP_K = [50, 500, 10, 1]          # register kernel, streaming kernel (k = V: off), register kernel, greedy
SEED, OFFSET = 2 ** 63 + 2 ** 32 + 11, 2 ** 40 + 3


@pytest.fixture(scope='module')
def tiny(nat):
    import guided_sampling_cases as G
    import masked_sampling_cases as M
    from oracle import configs as C
    ar, aux = M.model(C.RQT_TINY, 41, DEV)
    cond = M.cond_for(C.RQT_TINY, 4, DEV)
    ar._draw_rng = lambda device, n: (SEED, OFFSET)          # the (seed, offset) sample() would take from the generator
    return ar, aux, cond, G.uncond_for(C.RQT_TINY, cond)


def test_engine_sample_draws_certified_winners(nat, tiny):
    """RQTransformer.sample, B = 4, 4x4x4 codes: each code is the certified winner of its step's logits under counter
    offset + pos D + d, row field = the image's row"""
    ar, aux, cond, _ = tiny
    zeros = torch.zeros((4, 4, 4, 4), dtype=torch.long, device=DEV)
    out = ar.sample(zeros, aux, cond=cond, temperature=0.9, top_k=ENGINE_TOP_K)
    logits = ar.teacher_forced_logits(out, aux, cond=cond)
    for d, v in enumerate(ar.vocab_size):
        logits[..., d, v:] = float('-inf')
    worst, near = sc.certify_engine(out.cpu().numpy(), logits.cpu().numpy(), 0.9, ENGINE_TOP_K, SEED, OFFSET, 'sample')
    print(f'sample: 256 codes certified, largest deficit {worst:.3g} u, runner-up inside the tolerance in {near} steps')


def test_engine_sample_guided_draws_certified_winners(nat, tiny):
    """RQTransformer.sample_guided at scale 3: each code is the certified winner of the guided logits of its step, which the
    teacher-forced pass over cat(codes, codes) reproduces only if both twins received every code"""
    import guided_sampling_cases as G
    ar, aux, cond, uncond = tiny
    zeros = torch.zeros((4, 4, 4, 4), dtype=torch.long, device=DEV)
    out = ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=3.0, temperature=0.9, top_k=ENGINE_TOP_K)
    g = G.guided_step_logits(nat, ar, aux, out, cond, uncond, 3.0)
    worst, near = sc.certify_engine(out.cpu().numpy(), g.cpu().numpy(), 0.9, ENGINE_TOP_K, SEED, OFFSET, 'sample_guided')
    print(f'sample_guided: 256 codes certified, largest deficit {worst:.3g} u, runner-up inside the tolerance in {near} steps')
    # a twin that kept its own codes would see other logits from the second position on: the certificate above would fail there
    assert not torch.equal(out, ar.sample(zeros, aux, cond=cond, temperature=0.9, top_k=ENGINE_TOP_K))
