"""CPU-only: the C-ABI library builds for gfx950, loads, and exports every symbol include/rqamd.h
declares; the binding refuses to run without it (no CPU fallback).  No compute calls here."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.fixture(scope='module')
def lib_path():
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from rqvae import _native
    return _native.LIB_PATH


def test_header_symbols_exported(lib_path):
    header = open(os.path.join(ROOT, 'include', 'rqamd.h')).read()
    declared = set(re.findall(r'\b(rqamd_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 17
    lib = ctypes.CDLL(lib_path)
    for name in sorted(declared):
        assert hasattr(lib, name), f'{name} declared in include/rqamd.h but not exported'
    from rqvae import _native
    assert declared == set(_native.EXPORTS)
    lib.rqamd_abi_version.restype = ctypes.c_int
    assert lib.rqamd_abi_version() == _native.ABI_VERSION == 7
    # the fp16 build of the RQ-Transformer engine (sample(amp=True)): the rqamd_rqt_* subset of the same ABI
    assert os.path.exists(_native.LIB16_PATH)
    lib16 = ctypes.CDLL(_native.LIB16_PATH)
    for name in _native.EXPORTS_F16:
        assert hasattr(lib16, name), f'{name} missing from librqamd_f16.so'
    assert {n for n in declared if n.startswith('rqamd_rqt_')} <= set(_native.EXPORTS_F16)
    lib16.rqamd_abi_version.restype = ctypes.c_int
    assert lib16.rqamd_abi_version() == _native.ABI_VERSION


def test_status_codes_without_gpu(lib_path):
    """argument validation happens before any HIP call, so it is observable on a GPU-less host"""
    lib = ctypes.CDLL(lib_path)
    lib.rqamd_last_error.restype = ctypes.c_char_p
    assert lib.rqamd_rqt_create(None, None) == -1
    assert b'null' in lib.rqamd_last_error()
    from rqvae._native import RqtConfig
    cfg = RqtConfig(100, 3, 1, 1, 10, 64, 1, 1, 8, 8, 4, 0)          # embed_dim not a multiple of n_head (attentions.py:46 asserts)
    h = ctypes.c_void_p()
    assert lib.rqamd_rqt_create(ctypes.byref(cfg), ctypes.byref(h)) == -2
    assert b'head_dim' in lib.rqamd_last_error()
    cfg = RqtConfig(1024, 2, 1, 1, 10, 64, 1, 1, 8, 8, 4, 0)         # head_dim 512 > 256
    assert lib.rqamd_rqt_create(ctypes.byref(cfg), ctypes.byref(h)) == -2
    assert b'head_dim' in lib.rqamd_last_error()
    assert lib.rqamd_rqt_set_option(None, b'head.n_head', 2) == -1
    assert lib.rqamd_vae_decode(None, None, 1, None, None) == -1
    lib.rqamd_rq_quantize.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p]
    assert lib.rqamd_rq_quantize(None, None, None, None, 4, 0, 256, None, None, None, 0, None) == 0     # empty input is a no-op


def test_rqt_attn_diagnostics_refuse_without_gpu(lib_path):
    """rqamd_dbg_rqt_attn_decode / _prefill / _packed refuse, before any HIP call, whatever would make a kernel trap or write outside its
    buffers -- and the launchers' own refusals pass through with their messages.  Every call here is refused: the pointers are never read."""
    from rqvae import _native
    lib = _native._bind(lib_path)
    err = lambda: lib.rqamd_last_error().decode()
    p = ctypes.c_void_p(4096)                                   # any non-null value

    def dec(qkv=p, kc=p, vc=p, ksc=None, vsc=None, rows=2, nh=3, E=192, Tcap=64, t=5, t_max=63, step=None, y=p):
        return lib.rqamd_dbg_rqt_attn_decode(qkv, kc, vc, ksc, vsc, rows, nh, E, Tcap, t, t_max, step, 0, y, None)
    for kw, word in ((dict(qkv=None), 'null'), (dict(y=None), 'null'), (dict(rows=0), 'rows 0'), (dict(nh=0), 'n_head 0'), (dict(Tcap=0), 'Tcap 0'),
                     (dict(E=0), 'embed_dim 0'), (dict(t=-1), 't -1 outside'), (dict(t=64), 't 64 outside'), (dict(t=63, t_max=64), 't_max 64'),
                     (dict(t=9, t_max=8), 't 9 > t_max 8'), (dict(t=8, t_max=7), 't 8 > t_max 7'), (dict(vc=None), 'value cache'),
                     (dict(kc=None), 'key cache'), (dict(vsc=p), 'without key scales'), (dict(t=0, t_max=0, step=p, Tcap=0), 'Tcap 0')):
        assert dec(**kw) == -1, kw
        assert word in err(), (kw, err())
    # the launcher's refusals, unchanged
    for kw, word in ((dict(ksc=p, Tcap=320, t_max=319), 'end at 256 keys'), (dict(ksc=p, vsc=p, Tcap=320, t_max=100), 'end at 256 keys'),
                     (dict(nh=1, E=257), 'head_dim 257 > 256'), (dict(nh=3, E=240, Tcap=257, t_max=256), 'context 257 > 256'),
                     (dict(nh=3, E=240, ksc=p), 'written for head_dim 64'), (dict(nh=3, E=100), 'not a multiple of n_head')):
        assert dec(**kw) in (-1, -2), kw
        assert word in err(), (kw, err())
    assert dec(nh=3, E=100) == -1 and dec(nh=1, E=257) == -2

    def pre(qkv=p, kc=p, vc=p, ksc=None, vsc=None, n_img=2, P=4, nh=3, E=192, Tcap=8, y=p):
        return lib.rqamd_dbg_rqt_attn_prefill(qkv, kc, vc, ksc, vsc, n_img, P, nh, E, Tcap, y, None)
    for kw, code, word in ((dict(qkv=None), -1, 'null'), (dict(y=None), -1, 'null'), (dict(n_img=0), -1, '0 images'), (dict(nh=0), -1, 'n_head 0'),
                           (dict(vsc=p), -1, 'without key scales'), (dict(vc=None), -1, 'without a value cache'),
                           (dict(kc=None), -1, 'cache-free form with a cache pointer'), (dict(kc=None, vc=None, ksc=p), -1, 'cache-free form'),
                           (dict(P=9), -2, '9 tokens (cache 8)'), (dict(P=0), -2, '0 tokens'), (dict(P=256, Tcap=256, ksc=p), -2, '255 prefix tokens'),
                           (dict(P=256, Tcap=256, ksc=p, vsc=p), -2, '255 prefix tokens'), (dict(E=240, P=9), -2, '9 tokens (cache 8)'),
                           (dict(E=240, Tcap=257), -2, 'context 257 > 256'), (dict(E=240, ksc=p), -2, 'written for head_dim 64'),
                           (dict(nh=1, E=257), -2, 'head_dim 257 > 256')):
        assert pre(**kw) == code, kw
        assert word in err(), (kw, err())

    def pack(qkv=p, rows=16, group=4, nh=2, E=128, y=p):
        return lib.rqamd_dbg_rqt_attn_packed(qkv, rows, group, nh, E, y, None)
    for kw, code, word in ((dict(qkv=None), -1, 'null'), (dict(y=None), -1, 'null'), (dict(group=9, rows=18), -1, '18 rows in groups of 9'),
                           (dict(group=0), -1, 'groups of 0'), (dict(rows=17), -1, '17 rows in groups of 4'), (dict(rows=0), -1, '0 rows'),
                           (dict(nh=0), -1, 'n_head 0'), (dict(nh=3, E=128), -1, 'not a multiple'), (dict(nh=1, E=257), -2, 'head_dim 257 > 256')):
        assert pack(**kw) == code, kw
        assert word in err(), (kw, err())


def test_no_cpu_fallback(lib_path, monkeypatch):
    from rqvae import _native
    with pytest.raises(_native.RqamdError, match='CPU'):
        _native.ptr(torch.zeros(4))
    monkeypatch.setattr(_native, '_lib', None)
    monkeypatch.setattr(_native, 'LIB_PATH', '/nonexistent/librqamd.so')
    with pytest.raises(_native.RqamdError, match='no CPU fallback'):
        _native.lib()


def test_binding_has_no_host_pointer_switch():
    """the emulator tests swap the library / pointer marshalling from OUTSIDE (tests/emu/emu_binding.py); the shipped
    binding itself has no flag or entry point that accepts host memory"""
    src = open(os.path.join(ROOT, 'rq-vae-transformer_amd', 'rqvae', '_native.py')).read()
    assert '_allow_host_pointers' not in src and '_load_for_testing' not in src


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, 'rq-vae-transformer_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h')):
                src = open(os.path.join(dirpath, f)).read()
                assert 'import oracle' not in src and 'from oracle' not in src, f
