"""The certificate checks of tests/sampler_check.py on the host emulator (tests/emu): the same checker, case builders and tolerances as
the `-m gpu` twin (tests/test_gpu_sampler.py), on the subset small enough for fibers -- V <= 1024 with at most 8 rows per case, the
256 / 257 rows inside one bf16 bucket, the +-0.0 rows, every top-p edge, masks and temperatures, the stream cases (every seed x offset
at V = 64, over 300 rows unfiltered and 20 filtered; row seeds, a mixed per-row table) and, marked `slow`, the V = 4096 rows at and one past SMP_CAP.  The emulator
runs the kernels' own fp32 operation order with the host's logf / expf, so the checker is proven on the real kernel source before any
GPU time is spent; what the native __logf does to the streaming kernel's tail only the MI355X shows."""
import os
import sys

import numpy as np
import pytest

import sampler_check as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
EMU_ROWS = 8


@pytest.fixture(scope='module')
def nat():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'emu'))
    import build_emu
    path = build_emu.build()
    from rqvae import _native
    import emu_binding
    saved = emu_binding.install(_native, path)
    yield _native
    emu_binding.restore(_native, saved)


def _run(nat, case):
    case = case._replace(rows=min(case.rows, EMU_ROWS))
    x = sc.build_logits(case)
    worst, near, flags = sc.run_scalar_case(nat, x, case.T, case.k, case.p, case.seed, case.offset, 'cpu', case.name)
    print(f'{case.name}: largest deficit {worst:.3g} u, rows with a runner-up inside the tolerance {near} of {case.rows}')
    return flags


@pytest.mark.parametrize('case', [c for c in sc.CASES if c.emu == 1], ids=lambda c: c.name)
def test_emu_sampler_case(nat, case):
    _run(nat, case)


@pytest.mark.slow
@pytest.mark.parametrize('case', [c for c in sc.CASES if c.emu == 2], ids=lambda c: c.name)
def test_emu_sampler_cap(nat, case):
    """k = SMP_CAP distinct keys stay in the register kernel, k = SMP_CAP + 1 are handed to the general kernel"""
    flags = _run(nat, case)
    assert (flags == int(case.k > sc.SMP_CAP)).all()


@pytest.mark.parametrize('case', sc.stream_cases(64, filtered_rows=20), ids=lambda c: c.name)
def test_emu_sampler_stream(nat, case):
    """high words of seed and offset, 300 rows (20 where a filter runs): certified against the Philox reference, not against another call"""
    x = sc.build_logits(case)
    sc.run_scalar_case(nat, x, case.T, case.k, case.p, case.seed, case.offset, 'cpu', case.name)


def test_emu_sampler_probe_row(nat):
    """the row whose draw depends on u at a word below 64 (sampler_check.PROBE): all three kernels"""
    x, seed, offset = sc.probe_logits()
    for k in (None, 2):
        sc.run_scalar_case(nat, x, 1.0, k, None, seed, offset, 'cpu', f'probe k={k}')


@pytest.mark.parametrize('V', [500, 7])
def test_emu_sampler_rows(nat, V):
    """rqamd_sample_logits_rows: the mixed table of per_image_sampling_cases, with the call's seed and with one seed per row"""
    import per_image_sampling_cases as P
    x, table = P.kernel_logits(V, V), P.kernel_table(V)
    sc.run_rows_case(nat, x, table, None, 2 ** 32 + 9, 2 ** 40 + 3, 'cpu', f'rows V{V}')
    seeds = [3, 2 ** 40 + 5, 3, 0, 7, 2 ** 62, 1, 2 ** 63 + 11, 2 ** 32, 2 ** 32 - 1, 15, 17]
    sc.run_rows_case(nat, x, table, seeds, 99, 0, 'cpu', f'row seeds V{V}')
    sc.run_rows_case(nat, x, table, seeds, 99, 2 ** 32 + 1, 'cpu', f'row seeds V{V} with an offset')
