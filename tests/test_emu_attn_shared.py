"""CPU-only: the shared-prompt decode attention alone (rqamd_dbg_rqt_attn_shared, csrc/rqt_attn_shared.hip) through the host emulator
(tests/emu: the same .hip sources executed by fibers), with the cases of tests/attn_shared_cases.py.  The authoritative runs are the
`-m gpu` ones (tests/test_gpu_attn_shared.py), which also cover the fp16 build; the emulator is built from the bf16 sources only."""
import os
import re
import subprocess
import sys

import pytest
import torch

import attn_shared_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'rq-vae-transformer_amd', 'csrc')
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')
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


# Trimmed against the GPU file (attn_shared_cases.exact_cases, thin): every Ps x fan x nh x Tcap_row, one (t, counter form) each in rotation --
# all of them inside every test.


@needs_clang
@pytest.mark.parametrize('Ps', S.PS)
def test_emu_shared_equals_plain_on_expanded_cache(nat, Ps):
    assert S.exact_cases(nat, DEV, Ps, thin=Ps) == len(S.FANS) * len(S.HEADS) * len(S.TCAPS)


@needs_clang
@pytest.mark.parametrize('which', ['small', 'reg'])
def test_emu_shared_fp64(nat, which):
    print('shared %s, observed c %.3f' % (which, S.fp64_case(nat, DEV, which)))


@needs_clang
def test_emu_shared_refusals(nat):
    S.refusals(nat, DEV, pytest)


# ---------------------------------------------------------------------------------------------- no scratch on gfx950
SHARED_KERNELS = ('attn_shared_kernel', 'attn_shared_small_kernel')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
@pytest.mark.parametrize('f16', [False, True])
def test_shared_kernels_use_no_scratch(f16, tmp_path):
    """every instantiation of the two kernels (4 / 8 / 16 / 32 blocks, the small form) keeps everything in
    registers on gfx950, in the bf16 and the fp16 build"""
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-I', CSRC,
           '-Rpass-analysis=kernel-resource-usage', '--cuda-device-only', '-c', os.path.join(CSRC, 'rqt_attn_shared.hip'),
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
    mine = {k: v for k, v in seen.items() if 'attn_shared' in k}
    for n in SHARED_KERNELS:
        assert any(n in k for k in mine), f'{n} not found in the resource-usage remarks'
    assert len(mine) == 5, sorted(mine)                 # 4 block counts + the small form
    assert all(v == 0 for v in mine.values()), mine
