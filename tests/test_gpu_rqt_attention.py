"""The RQ-Transformer's attention kernels alone on a real MI355X (`-m gpu`): rqamd_dbg_rqt_attn_decode / _prefill / _packed against fp64, with
the inputs, bound, side-effect checks and the full case list of tests/rqt_attn_cases.py (its docstring states the bound and lists the
observed c per kernel class; every test prints the values observed so far under -s).  Tensors are made on the CPU and moved to the device;
the fp64 references are computed on the device.  tests/test_emu_rqt_attention.py runs the same cases through the host emulator."""
import pytest
import torch

import rqt_attn_cases as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


@pytest.fixture(autouse=True)
def _report():
    yield
    print('gpu rqt attention, observed c so far: ' + R.report())


@pytest.mark.parametrize('fmt', R.FMTS)
@pytest.mark.parametrize('rows', R.SMALL_ROWS)
def test_gpu_decode_small(nat, rows, fmt):
    R.small_cases(nat, DEV, rows, fmt)


@pytest.mark.parametrize('fmt', R.FMTS)
@pytest.mark.parametrize('two', [False, True], ids=['one_head', 'two_heads'])
def test_gpu_decode_register(nat, two, fmt):
    R.reg_cases(nat, DEV, fmt, two)


@pytest.mark.parametrize('fmt', R.FMTS)
def test_gpu_decode_dynamic(nat, fmt):
    R.dyn_cases(nat, DEV, fmt)


@pytest.mark.parametrize('nw', [4, 1])
@pytest.mark.parametrize('Tcap', sorted(R.LONG_T))
def test_gpu_decode_long(nat, Tcap, nw):
    R.long_cases(nat, DEV, Tcap, nw, R.LONG_T[Tcap])


@pytest.mark.parametrize('nw', [4, 1])
def test_gpu_decode_long_low_scores(nat, nw):
    R.long_low_cases(nat, DEV, nw)


def test_gpu_decode_forced_long(nat, monkeypatch):
    print('largest |long - register| %.3e' % R.forced_long_vs_register(nat, DEV, monkeypatch.setenv))


@pytest.mark.parametrize('hd', R.GENERIC_HD)
def test_gpu_decode_generic(nat, hd):
    R.generic_cases(nat, DEV, hd)


@pytest.mark.parametrize('P', R.PREFILL_PLAIN + R.PREFILL_TILED)
def test_gpu_prefill(nat, P):
    R.prefill_cases(nat, DEV, P, 'tiled' if P > 255 else 'plain')


@pytest.mark.parametrize('fmt', ['int8k', 'int8kv'])
@pytest.mark.parametrize('P', R.PREFILL_INT8)
def test_gpu_prefill_8bit_append(nat, P, fmt):
    R.prefill_case(nat, DEV, 2, P, 3, P + 9, fmt=fmt, kind='peaked', expect='plain')
    R.prefill_case(nat, DEV, 2, P, 3, P, fmt=fmt, expect='plain')


@pytest.mark.parametrize('P', R.PREFILL_FORCED)
def test_gpu_prefill_forced_tiled_bit_identical(nat, P, monkeypatch):
    R.prefill_forced_tiled(nat, DEV, P, monkeypatch.setenv)


@pytest.mark.parametrize('hd,P', R.PREFILL_GENERIC)
def test_gpu_prefill_generic(nat, hd, P):
    for cache, kind in ((True, 'flat'), (False, 'peaked')):
        R.prefill_case(nat, DEV, 2, P, 3, P + 9 if P < 256 else P, cache=cache, kind=kind, hd=hd, expect='generic')


@pytest.mark.parametrize('hd,nh', R.PACKED)
def test_gpu_packed(nat, hd, nh):
    for group in range(1, 9):
        for kind in R.KINDS:
            R.packed_case(nat, DEV, group, nh, hd, kind, R.packed_branch(nh, nh * hd))
    assert R.packed_branch(nh, nh * hd) == {64: 'hd64', 32: 'vec', 20: 'scalar'}[hd]


@pytest.mark.parametrize('fmt', R.FMTS)
def test_gpu_append_special_keys(nat, fmt):
    R.append_special(nat, DEV, fmt)


def test_gpu_chain_vs_prefill(nat):
    R.chain_vs_prefill(nat, DEV)


@pytest.mark.parametrize('name,kw', R.CLASS_CASES, ids=[c[0] for c in R.CLASS_CASES])
def test_gpu_rows_independent_and_relaunch(nat, name, kw):
    R.rows_and_relaunch(nat, DEV, name, kw)


def test_gpu_refusals(nat):
    R.refusals(nat, DEV, pytest)
