"""CPU-only: the RQ-Transformer's attention kernels alone (rqamd_dbg_rqt_attn_decode / _prefill / _packed) through the host emulator
(tests/emu: the same .hip sources executed by fibers) against fp64, with the inputs, bound, side-effect checks and case lists of
tests/rqt_attn_cases.py.  The authoritative runs are the `-m gpu` ones (tests/test_gpu_rqt_attention.py); this file proves the harness, the
guards and the dispatch assertions, and catches index errors, without a GPU.  The emulator's exp2f is the host's, so the observed c
(printed under -s) sits below the GPU's; the bound is the same.

Trimmed against the GPU file: the chunked decode kernel at Tcap 1088 runs t in {512, 1087} only (rqt_attn_cases.LONG_T_EMU); everything
else is the full list."""
import os
import sys

import pytest
import torch

import rqt_attn_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
DEV = torch.device('cpu')


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


@pytest.fixture(autouse=True)
def _report():
    yield
    print('emu rqt attention, observed c so far: ' + R.report())


@pytest.mark.parametrize('fmt', R.FMTS)
@pytest.mark.parametrize('rows', R.SMALL_ROWS)
def test_emu_decode_small(nat, rows, fmt):
    R.small_cases(nat, DEV, rows, fmt)


@pytest.mark.parametrize('fmt', R.FMTS)
@pytest.mark.parametrize('two', [False, True], ids=['one_head', 'two_heads'])
def test_emu_decode_register(nat, two, fmt):
    R.reg_cases(nat, DEV, fmt, two)


@pytest.mark.parametrize('fmt', R.FMTS)
def test_emu_decode_dynamic(nat, fmt):
    R.dyn_cases(nat, DEV, fmt)


@pytest.mark.parametrize('nw', [4, 1])
@pytest.mark.parametrize('Tcap', sorted(R.LONG_T_EMU))
def test_emu_decode_long(nat, Tcap, nw):
    R.long_cases(nat, DEV, Tcap, nw, R.LONG_T_EMU[Tcap])


@pytest.mark.parametrize('nw', [4, 1])
def test_emu_decode_long_low_scores(nat, nw):
    R.long_low_cases(nat, DEV, nw)


def test_emu_decode_forced_long(nat, monkeypatch):
    print('largest |long - register| %.3e' % R.forced_long_vs_register(nat, DEV, monkeypatch.setenv))


@pytest.mark.parametrize('hd', R.GENERIC_HD)
def test_emu_decode_generic(nat, hd):
    R.generic_cases(nat, DEV, hd)


@pytest.mark.parametrize('P', R.PREFILL_PLAIN + R.PREFILL_TILED)
def test_emu_prefill(nat, P):
    R.prefill_cases(nat, DEV, P, 'tiled' if P > 255 else 'plain')


@pytest.mark.parametrize('fmt', ['int8k', 'int8kv'])
@pytest.mark.parametrize('P', R.PREFILL_INT8)
def test_emu_prefill_8bit_append(nat, P, fmt):
    R.prefill_case(nat, DEV, 2, P, 3, P + 9, fmt=fmt, kind='peaked', expect='plain')
    R.prefill_case(nat, DEV, 2, P, 3, P, fmt=fmt, expect='plain')


@pytest.mark.parametrize('P', R.PREFILL_FORCED)
def test_emu_prefill_forced_tiled_bit_identical(nat, P, monkeypatch):
    R.prefill_forced_tiled(nat, DEV, P, monkeypatch.setenv)


@pytest.mark.parametrize('hd,P', R.PREFILL_GENERIC)
def test_emu_prefill_generic(nat, hd, P):
    for cache, kind in ((True, 'flat'), (False, 'peaked')):
        R.prefill_case(nat, DEV, 2, P, 3, P + 9 if P < 256 else P, cache=cache, kind=kind, hd=hd, expect='generic')


@pytest.mark.parametrize('hd,nh', R.PACKED)
def test_emu_packed(nat, hd, nh):
    for group in range(1, 9):
        for kind in R.KINDS:
            R.packed_case(nat, DEV, group, nh, hd, kind, R.packed_branch(nh, nh * hd))
    assert R.packed_branch(nh, nh * hd) == {64: 'hd64', 32: 'vec', 20: 'scalar'}[hd]


@pytest.mark.parametrize('fmt', R.FMTS)
def test_emu_append_special_keys(nat, fmt):
    R.append_special(nat, DEV, fmt)


def test_emu_chain_vs_prefill(nat):
    R.chain_vs_prefill(nat, DEV)


@pytest.mark.parametrize('name,kw', R.CLASS_CASES, ids=[c[0] for c in R.CLASS_CASES])
def test_emu_rows_independent_and_relaunch(nat, name, kw):
    R.rows_and_relaunch(nat, DEV, name, kw)


def test_emu_refusals(nat):
    R.refusals(nat, DEV, pytest)


FENCE = 64 * 4096


def _fenced(content):
    """`content` at the very end of an anonymous mapping whose next FENCE bytes are inaccessible: a load past its last element cannot
    return a value.  Returns (the mapping, to be kept alive; the tensor)."""
    import ctypes
    import mmap
    nbytes = content.numel() * content.element_size()
    body = -(-nbytes // mmap.PAGESIZE) * mmap.PAGESIZE
    m = mmap.mmap(-1, body + FENCE)
    addr = ctypes.addressof(ctypes.c_char.from_buffer(m))
    assert ctypes.CDLL(None, use_errno=True).mprotect(ctypes.c_void_p(addr + body), ctypes.c_size_t(FENCE), 0) == 0
    t = torch.frombuffer(m, dtype=content.dtype, count=content.numel(), offset=body - nbytes)
    t.copy_(content.reshape(-1))
    return m, t.view(content.shape)


@pytest.mark.parametrize('fmt', ['bf16', 'int8kv'])
def test_emu_decode_small_tail_loads_stay_inside(nat, fmt):
    """attn_small_kernel at 35 pairs: the 29 lanes groups past rows * nh mask their stores, so nothing they load shows in any output -- only
    where they load from tells whether they clamp.  Here qkv, both caches and both scale arrays end where inaccessible memory begins: the
    pair index of an unclamped group points up to 40 KB past the caches."""
    d = R.make_decode(7, 5, 64, 11, 3, fmt, 'flat', seed=35)
    assert R.decode_branch(7, 5, 320, 11, 7, fmt) == 'small'
    keep, t = {}, {}
    for name in ('qkv', 'kc', 'vc', 'ksc', 'vsc'):
        x = getattr(d, name)
        keep[name], t[name] = _fenced(x) if x is not None else (None, None)
    y = R.Buf(R.nan_like((7, 320)), DEV)
    nat.dbg_rqt_attn_decode(t['qkv'], t['kc'], t['vc'], y.t, 5, 11, 3, t_max=7, ksc=t['ksc'], vsc=t['vsc'])
    ref, A = R.attn_ref(d.q.double()[:, :, None], d.K, d.V)
    R.check(y.t.view(7, 5, 1, 64), ref, A, fmt, 'small', 'fenced small kernel')
    y.check_guard('fenced small kernel')
    for name in ('kc', 'vc'):
        assert R.same_bits(t[name][:, :, :3], getattr(d, name)[:, :, :3])
