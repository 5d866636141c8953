"""CPU-only checks of the one-pass prefix prefill ("prefix.one_pass", rqamd_rqt_step_prefill, RQTransformer.prefix_mode) through the
host emulator (tests/emu): the same .hip sources executed by fibers.  The cases are tests/prefix_prefill_cases.py, shared with the
authoritative `-m gpu` runs (tests/test_gpu_prefix_prefill.py)."""
import os
import re
import subprocess
import sys

import pytest

import prefix_prefill_cases as PC

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
    PC.forget_cases()
    emu_binding.restore(_native, saved)


# ---------------------------------------------------------------------------------------------- 1. logits after the prefill
@needs_clang
@pytest.mark.parametrize('n0', PC.TINY_N0)
def test_emu_prefill_logits_tiny(nat, golden, n0):
    PC.check_prefill_logits(PC.case(golden, 'tiny', DEV), n0, PC.REF_TINY, 'emu rqt_tiny')


@needs_clang
@pytest.mark.parametrize('n0', PC.TXT_N0)
def test_emu_prefill_logits_text_conditioned(nat, golden, n0):
    """4 conditioning tokens: the 3 text tokens of the prefix are part of the pass (3 + n0 tokens per image)"""
    PC.check_prefill_logits(PC.case(golden, 'txt', DEV), n0, PC.REF_TINY, 'emu rqt_tiny_txt')


@needs_clang
@pytest.mark.parametrize('tag', sorted(PC.VARIANTS))
def test_emu_prefill_logits_variants(nat, golden, tag):
    """tuple: learned token embeddings (body_input_kernel's table path); heads: head size 32 (the one-wavefront-per-token append);
    nocumsum"""
    PC.check_prefill_logits(PC.case(golden, tag, DEV), 9, PC.REF_TINY, f'emu variant {tag}')


# ---------------------------------------------------------------------------------------------- 2. chunking
@needs_clang
def test_emu_prefill_chunked(nat, golden):
    PC.check_chunked(PC.case(golden, 'tiny', DEV), PC.REF_TINY)


# ---------------------------------------------------------------------------------------------- 3. long contexts and cache formats
@needs_clang
@pytest.mark.parametrize('n0', [1, 8, 15])
def test_emu_prefill_long_text(nat, golden, n0):
    """rqt_long_txt300: 300 .. 314 tokens per image, text then codes, through the tiled append"""
    PC.check_prefill_logits(PC.case(golden, 'txt300', DEV), n0, PC.REF_LONG['emu'], 'emu rqt_long_txt300')


@needs_clang
@pytest.mark.parametrize('fmt', ['int8k', 'int8kv'])
def test_emu_prefill_int8_cache(nat, golden, monkeypatch, fmt):
    monkeypatch.setenv('RQAMD_KV', fmt)
    PC.check_prefill_logits(PC.case(golden, 'tiny', DEV), 9, PC.REF_INT8['emu'], f'emu rqt_tiny, {fmt} cache')


# ---------------------------------------------------------------------------------------------- 4.-9. the sampling forms
@needs_clang
def test_emu_forms_agree_and_draws_see_the_prefix(nat):
    ar, aux, cond, partial, codes, lp = PC.check_forms_agree(DEV)
    PC.check_conditioned_on_prefix(ar, aux, cond, partial, codes, lp)


@needs_clang
def test_emu_stale_cache(nat):
    PC.check_stale_cache(DEV)


@needs_clang
def test_emu_errors(nat):
    PC.check_errors(nat, DEV)


@needs_clang
def test_emu_default_untouched(nat):
    PC.check_default_untouched(DEV)


@needs_clang
def test_emu_cached_forward_restart(nat):
    PC.check_cached_forward_restart(DEV)


def test_prefix_mode_default_and_env(monkeypatch):
    from oracle import configs as C
    from rqvae.models.rqtransformer import RQTransformer
    monkeypatch.delenv('RQAMD_PREFIX', raising=False)
    assert RQTransformer(C.RQT_TINY).prefix_mode == 'stepped'
    monkeypatch.setenv('RQAMD_PREFIX', 'one_pass')
    assert RQTransformer(C.RQT_TINY).prefix_mode == 'one_pass'


# ---------------------------------------------------------------------------------------------- no scratch on gfx950
PREFIX_KERNELS = ('gather_codes_kernel', 'body_input_kernel')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
@pytest.mark.parametrize('f16', [False, True])
def test_prefix_kernels_use_no_scratch(f16, tmp_path):
    """the two input kernels with their positions-per-image count (the only device code the prefill changes) keep everything in registers
    on gfx950, in the bf16 and the fp16 build; the appending attention kernels it drives are unchanged"""
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-I', CSRC,
           '-Rpass-analysis=kernel-resource-usage', '--cuda-device-only', '-c', os.path.join(CSRC, 'rqt_kernels.hip'),
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
    mine = {k: v for k, v in seen.items() if any(n in k for n in PREFIX_KERNELS)}
    for n in PREFIX_KERNELS:
        assert any(n in k for k in mine), f'{n} not found in the resource-usage remarks'
    assert all(v == 0 for v in mine.values()), mine
    src = open(os.path.join(CSRC, 'rqt_kernels.h')).read()
    assert re.search(r'struct GatherCodesArgs \{[^}]*\bn_pos;', src) and re.search(r'struct BodyInputArgs \{[^}]*\bn_pos;', src)
