"""The residual quantiser (csrc/quantize.hip) certified against fp64 on the MI355X in every launch form, with the checks of
tests/quantiser_check.py (the evidence that they can fail is tests/test_quantiser_check.py; the emulator twin is
tests/test_emu_quantiser.py): all four dims, one to four and more ring steps (the partly primed ring and every branch of the counted
wait), K = 1 and K < 4, ragged and multi-workgroup vector counts, the codebook-split form at every dim with ragged K, unshared
codebooks, a last split of one code and the 64-split cap -- each split case once more as a single launch, bit-identical --
constructed ties across lanes, code groups, tiles and splits, residual-like inputs, and rq_distances / rq_soft_codes / rq_code_norms.
Nothing is left out of the code check: every vector and depth carries the certificate d64[k] - E[k] <= min_j (d64[j] + E[j]).
Inputs sit in NaN-poisoned buffers, outputs are views into guard-filled ones.  Run with -s for the observed ratios."""
import pytest
import torch

import quantiser_check as qc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# observed on MI355X (printed under -s; for information, no bound is derived from these):
#   rq_distances max err / (u n S): dim 64 0.0502 (the 40000 x 129 matrix; K = 77: 0.0268, K = 1153: 0.0411), dim 128 0.0205, dim 192
#   0.0121, dim 256 0.0106 -- against C_CHAIN 0.2988 / 0.1936 / 0.1244 / 0.1192 and the derived ceiling 1
#   certificate allowance used: 0 in every case (every code is the fp64 argmin of its teacher-forced residual)


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    yield _native
    for key in sorted(qc.OBSERVED):
        print(f'\nquantiser: {key:20s} largest observed ratio {qc.OBSERVED[key]:.4g}', end='')
    print(f'\nquantiser: C_CHAIN {qc.C_CHAIN}, KAPPA {qc.KAPPA}')


def _ids(c):
    return c.name


@pytest.mark.parametrize('case', qc.SINGLE_CASES, ids=_ids)
def test_single_launch(nat, case):
    """K < 1024: all depths in one launch"""
    assert qc.split_plan(case.n_vec, case.ks) is None
    used = qc.run_quantize_case(nat, case, DEV)
    print(f'{case.name}: ring steps {[qc.nstep(K, case.dim) for K in case.ks]}, certificate allowance used {used:.3g}')


@pytest.mark.parametrize('case', qc.SPLIT_CASES, ids=_ids)
def test_split_form_and_its_single_launch(nat, case):
    """K >= 1024 on fewer than 96 vector tiles: the codebook divided over blockIdx.y + the combine kernel; then the same vectors under
    dbg_set_row_scale(96) as one launch: codes and quants bit-identical"""
    plan = qc.split_plan(case.n_vec, case.ks)
    assert plan is not None
    used = qc.run_quantize_case(nat, case, DEV, other_form=True)
    print(f'{case.name}: (tiles per split, splits) {plan}, certificate allowance used {used:.3g}')


@pytest.mark.parametrize('case', qc.TIE_CASES, ids=_ids)
def test_ties_go_to_the_lowest_index(nat, case):
    """exact duplicate rows have bit-equal kernel distances: the lowest index wins across lanes, code groups, tiles and splits, in
    both launch forms; a codebook of identical rows gives code 0 everywhere"""
    qc.run_quantize_case(nat, case, DEV, other_form=case.split)


@pytest.mark.parametrize('case', qc.DIST_CASES, ids=_ids)
def test_distances(nat, case):
    ratio = qc.run_distance_case(nat, case, DEV)
    print(f'{case.name}: max err / (u n S) = {ratio:.4f}  (C_CHAIN {qc.C_CHAIN[case.dim]:.4f}, ceiling 1)')


@pytest.mark.parametrize('case', qc.SOFT_CASES, ids=_ids)
def test_soft_codes(nat, case):
    seen = qc.run_soft_case(nat, case, DEV)
    print(f'{case.name}: max |soft - p64| / bound = {seen:.4f}  (KAPPA {qc.KAPPA[case.dim]:.3g})')
