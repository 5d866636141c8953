"""CPU-only: the cache-extending causal attention alone (rqamd_dbg_rqt_attn_extend, csrc/rqt_attn_extend.hip) through the host emulator
(tests/emu): the same .hip source executed by fibers.  The cases are tests/attn_extend_cases.py, shared with the authoritative `-m gpu`
run (tests/test_gpu_attn_extend.py); the fp16 build exists on the GPU only."""
import os
import re
import subprocess
import sys

import pytest

import attn_extend_cases as X
import rqt_attn_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'rq-vae-transformer_amd', 'csrc')
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
DEV = 'cpu'


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


@needs_clang
@pytest.mark.parametrize('case', X.CASES, ids=X.case_id)
def test_emu_extend_bit_identical_to_prefill(nat, case):
    X.bit_identity(nat, DEV, case, 'peaked' if case[0] == 256 else 'flat')


@needs_clang
@pytest.mark.parametrize('kind', X.KINDS)
@pytest.mark.parametrize('case', X.FP64_CASES[:3], ids=X.case_id)
def test_emu_extend_vs_fp64(nat, case, kind):
    """(Tcap 1088 runs in the bit-identity test here and against fp64 on the GPU: 1088 keys x 88 queries of fibers twice over is slow)"""
    X.fp64_check(nat, DEV, case, kind)
    print('emu extend attention, observed c so far: ' + R.report())


@needs_clang
def test_emu_extend_refusals(nat):
    X.refusals(nat, DEV, pytest)


def test_extend_is_bound_in_both_builds():
    from rqvae import _native
    for name in ('rqamd_dbg_rqt_attn_extend', 'rqamd_rqt_step_run'):
        assert name in _native.EXPORTS and name in _native.EXPORTS_F16
    hdr = open(os.path.join(ROOT, 'include', 'rqamd.h')).read()
    assert 'int rqamd_dbg_rqt_attn_extend(const void* qkv, void* kc, void* vc, int n_img, int R, int T0,' in re.sub(r'\s+', ' ', hdr)
    assert 'int rqamd_rqt_step_run(rqamd_rqt* h, int p0, int p1, void* stream);' in hdr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
@pytest.mark.parametrize('f16', [False, True])
def test_extend_kernel_uses_no_scratch(f16, tmp_path):
    """lane = query keeps 64 query components and 64 accumulators per lane: they must stay in registers on gfx950, in both builds"""
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-I', CSRC,
           '-Rpass-analysis=kernel-resource-usage', '--cuda-device-only', '-c', os.path.join(CSRC, 'rqt_attn_extend.hip'),
           '-o', str(tmp_path / 'k.o')] + (['-DRQ_F16=1'] if f16 else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    seen, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
        m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', line)
        if m and name:
            seen[name] = int(m.group(1))
    mine = {k: v for k, v in seen.items() if 'attn_extend_kernel' in k}
    assert mine, 'attn_extend_kernel not found in the resource-usage remarks'
    assert all(v == 0 for v in mine.values()), mine
