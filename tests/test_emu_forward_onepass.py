"""CPU-only checks of the one-pass teacher-forced forward (rqamd_rqt_forward_onepass / rqamd_rqt_log_probs) through the host
emulator (tests/emu): the same .hip sources executed by fibers, against the reference-generated golden fixtures and the oracle.
The authoritative runs are the `-m gpu` ones (tests/test_gpu_forward_onepass.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import configs as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'rq-vae-transformer_amd', 'csrc')
CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
needs_clang = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')

VARIANTS = {'tuple': 'RQT_TINY_TUPLE', 'nocumsum': 'RQT_TINY_NOCUMSUM', 'mixed': 'RQT_TINY_MIXED', 'nobias': 'RQT_TINY_NOBIAS',
            'gelumix': 'RQT_TINY_GELUMIX', 'heads': 'RQT_TINY_HEADS', 'txtheads': 'RQT_TINY_TXT_HEADS'}


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


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rqt_engine(nat, cfg, params):
    eng = nat.RqtEngine(embed_dim=cfg['embed_dim'], n_head=cfg['body']['block']['n_head'], n_layer_body=cfg['body']['n_layer'],
                        n_layer_head=cfg['head']['n_layer'], vocab_size=cfg['vocab_size'], input_embed_dim=cfg['input_embed_dim'],
                        vocab_size_cond=cfg['vocab_size_cond'], block_size_cond=cfg['block_size_cond'],
                        block_size=cfg['block_size'], gelu_v2=cfg.get('gelu', 'v1') == 'v2', device='cpu')
    for k, v in params.items():
        eng.set_param(k, T(v))
    return eng


def _tiny(nat, golden, name='rqt_tiny.npz', cfg=None):
    g = golden(name)
    cfg = cfg or C.RQT_TINY
    hps, dd = C.VAE_TINY
    cb = oracle.make_params(oracle.rqvae_param_shapes(hps, dd), int(g['vae_seed']))['quantizer.codebooks.0.weight'][:-1]
    params = oracle.make_params(oracle.rqt_param_shapes(cfg), int(g['seed']))
    eng = _rqt_engine(nat, cfg, params)
    return g, cfg, params, cb, eng


def _bounds(got, want, what):
    err = np.abs(got - want)
    print('emu one-pass %s: max err %.4f mean err %.5f' % (what, err.max(), err.mean()))
    assert err.max() < 0.06 and err.mean() < 0.01, what          # the bounds of the stepped emulator tests on the same fixtures


def _variant_model(golden, tag):
    from rqvae.models.rqtransformer import RQTransformer
    from rqvae.models.rqvae import RQVAE
    g = golden(f'rqt_var_{tag}.npz')
    cfg = getattr(C, VARIANTS[tag])
    hps, dd = C.VAE_TINY
    vae = RQVAE(**hps, ddconfig=dd, checkpointing=False)
    vae.load_state_dict({k: T(v) for k, v in oracle.make_params(oracle.rqvae_param_shapes(hps, dd), int(g['vae_seed'])).items()})
    ar = RQTransformer(cfg).eval()
    ar.load_state_dict({k: T(v) for k, v in oracle.make_params(oracle.rqt_param_shapes(cfg), int(g['seed']), cfg).items()}, strict=True)
    return g, ar, (vae if tag != 'tuple' else None)


# ---------------------------------------------------------------------------------------------- 1. against the fixtures
@needs_clang
def test_emu_onepass_tiny_logits(nat, golden):
    g, cfg, params, cb, eng = _tiny(nat, golden)
    codes, cond = T(g['codes'].astype(np.int64)), T(g['cond'].astype(np.int64))
    logits = eng.forward_onepass(codes, cond, [T(cb)] * 4).numpy()
    _bounds(logits, g['logits'], 'rqt_tiny')
    stepped = eng.logits(codes, cond, [T(cb)] * 4).numpy()
    print('emu one-pass rqt_tiny: max diff to the stepped path %.5f' % np.abs(logits - stepped).max())
    assert np.abs(logits - stepped).max() < 0.02                 # same arithmetic, other GEMM tiles
    # the large-row kernel variants (chosen by the row count) on these few rows
    nat.dbg_set_row_scale(4096)
    try:
        big = eng.forward_onepass(codes, cond, [T(cb)] * 4).numpy()
    finally:
        nat.dbg_set_row_scale(1)
    _bounds(big, g['logits'], 'rqt_tiny, large-batch kernel variants')


@needs_clang
def test_emu_onepass_text_conditioned(nat, golden):
    g, cfg, params, cb, eng = _tiny(nat, golden, 'rqt_tiny_txt.npz', C.RQT_TINY_TXT)
    codes, cond = g['codes'].astype(np.int64), g['cond'].astype(np.int64)
    seq, cl = eng.forward_onepass(T(codes), T(cond), [T(cb)] * 4)
    _bounds(seq.numpy(), g['logits'], 'rqt_tiny_txt')
    ref = oracle.RQTransformerOracle(cfg, params).forward(codes, [cb] * 4, cond, return_cond_logits=True)
    _bounds(cl.numpy(), ref[1], 'rqt_tiny_txt cond_logits')


@needs_clang
@pytest.mark.parametrize('tag', sorted(VARIANTS))
def test_emu_onepass_flag_variants(nat, golden, tag):
    g, ar, vae = _variant_model(golden, tag)
    ar.forward_mode = 'one_pass'
    codes, cond = T(g['codes'].astype(np.int64)), T(g['cond'].astype(np.int64))
    logits = ar(codes, vae, cond=cond)
    logits = (logits[0] if isinstance(logits, tuple) else logits).numpy()
    _bounds(logits, g['logits'], f'variant {tag}')
    tf = ar.teacher_forced_logits(codes, vae, cond=cond).numpy()
    assert np.array_equal(tf, logits)
    ar.forward_mode = 'stepped'
    st = ar(codes, vae, cond=cond)
    st = (st[0] if isinstance(st, tuple) else st).numpy()
    assert np.abs(st - logits).max() < 0.02


def _long_prefix():
    cfg = C.rqt(128, 2, 1, 1, 500, vocab_cond=20, block_cond=70, block_size=(4, 4, 4), input_embed_dim=64)
    params = oracle.make_params(oracle.rqt_param_shapes(cfg), 43)
    rng = np.random.default_rng(44)
    cb = rng.standard_normal((500, 64), dtype=np.float32)
    codes, cond = rng.integers(0, 500, (2, 4, 4, 4)), rng.integers(0, 20, (2, 70))
    return cfg, params, cb, codes, cond


@needs_clang
def test_emu_onepass_long_prefix(nat):
    """70 conditioning tokens: 85 body tokens per image, i.e. two query blocks of the cache-free causal attention."""
    cfg, params, cb, codes, cond = _long_prefix()
    eng = _rqt_engine(nat, cfg, params)
    seq, cl = eng.forward_onepass(T(codes), T(cond), [T(cb)] * 4)
    ref = oracle.RQTransformerOracle(cfg, params).forward(codes, [cb] * 4, cond, return_cond_logits=True)
    _bounds(seq.numpy(), ref[0], 'long prefix')
    _bounds(cl.numpy(), ref[1], 'long prefix cond_logits')


def _depth1():
    cfg = C.rqt(128, 2, 2, 0, 500, vocab_cond=10, block_size=(4, 4, 1), input_embed_dim=64)
    params = oracle.make_params(oracle.rqt_param_shapes(cfg), 45)
    rng = np.random.default_rng(46)
    cb = rng.standard_normal((500, 64), dtype=np.float32)
    codes, cond = rng.integers(0, 500, (3, 4, 4, 1)), rng.integers(0, 10, (3, 1))
    return cfg, params, cb, codes, cond


@needs_clang
def test_emu_onepass_depth1_no_head_stack(nat):
    cfg, params, cb, codes, cond = _depth1()
    eng = _rqt_engine(nat, cfg, params)
    logits = eng.forward_onepass(T(codes), T(cond), [T(cb)]).numpy()
    ref = oracle.RQTransformerOracle(cfg, params).forward(codes, [cb], cond)
    _bounds(logits, ref, 'depth 1, no head stack')
    lp = eng.log_probs(T(codes), T(cond), [T(cb)]).numpy()
    want = _logp64(logits, codes)
    assert np.abs(lp - want).max() < LOGP_BOUND


# ---------------------------------------------------------------------------------------------- 2. several ragged chunks
@needs_clang
def test_emu_onepass_chunked(nat, golden):
    """fwd.chunk_rows forced small: 7 images (the fixture's tiled) in body chunks of 3 + 3 + 1 images, head sub-chunks of 5
    positions (48 per body chunk: 9 full ones and a ragged one of 3)."""
    g, cfg, params, cb, eng = _tiny(nat, golden)
    n = g['codes'].shape[0]
    idx = np.arange(7) % n
    codes, cond = g['codes'].astype(np.int64)[idx], g['cond'].astype(np.int64)[idx]
    eng.set_option('fwd.chunk_rows', 3 * 16)         # 16 body tokens per image (block_size_cond = 1)
    eng_h = eng
    logits = eng_h.forward_onepass(T(codes), T(cond), [T(cb)] * 4).numpy()
    _bounds(logits, g['logits'][idx], 'rqt_tiny, body chunks 3 + 3 + 1')
    eng.set_option('fwd.chunk_rows', 20)             # one image per body chunk (16 rows), 5 positions per head sub-chunk: 3 + 1 ragged
    logits2 = eng.forward_onepass(T(codes), T(cond), [T(cb)] * 4).numpy()
    _bounds(logits2, g['logits'][idx], 'rqt_tiny, one image per chunk, ragged head sub-chunks')
    lp = eng.log_probs(T(codes), T(cond), [T(cb)] * 4).numpy()
    assert np.abs(lp - _logp64(logits2, codes)).max() < LOGP_BOUND
    with pytest.raises(ValueError):
        eng.set_option('fwd.chunk_rows', 0)
    # text-conditioned: 4 + 16 - 1 = 19 body tokens per image
    gt, cfgt, pt, cbt, engt = _tiny(nat, golden, 'rqt_tiny_txt.npz', C.RQT_TINY_TXT)
    nt = gt['codes'].shape[0]
    idx = np.arange(5) % nt
    codes, cond = gt['codes'].astype(np.int64)[idx], gt['cond'].astype(np.int64)[idx]
    Tb = cfgt['block_size_cond'] - 1 + 16
    engt.set_option('fwd.chunk_rows', 2 * Tb + 3)    # chunks of 2 + 2 + 1 images
    seq, cl = engt.forward_onepass(T(codes), T(cond), [T(cbt)] * 4)
    _bounds(seq.numpy(), gt['logits'][idx], 'rqt_tiny_txt, body chunks 2 + 2 + 1')
    ref = oracle.RQTransformerOracle(cfgt, pt).forward(codes, [cbt] * 4, cond, return_cond_logits=True)
    _bounds(cl.numpy(), ref[1], 'rqt_tiny_txt cond_logits, chunked')


# ---------------------------------------------------------------------------------------------- 3. causality, bit for bit
@needs_clang
def test_emu_onepass_causality_and_determinism(nat, golden):
    g, cfg, params, cb, eng = _tiny(nat, golden)
    codes, cond = g['codes'].astype(np.int64), g['cond'].astype(np.int64)
    cbs = [T(cb)] * 4
    (B, H, W, D) = codes.shape
    V = cfg['vocab_size']
    base = eng.forward_onepass(T(codes), T(cond), cbs).numpy().reshape(B, H * W, D, -1)
    again = eng.forward_onepass(T(codes), T(cond), cbs).numpy().reshape(B, H * W, D, -1)
    assert np.array_equal(base, again)                               # two calls are bit-identical
    for q in (0, 5, H * W - 1):
        ch = codes.reshape(B, H * W, D).copy()
        ch[:, q, :] = (ch[:, q, :] + 1 + np.arange(D)) % V           # every depth of position q
        out = eng.forward_onepass(T(ch.reshape(codes.shape)), T(cond), cbs).numpy().reshape(B, H * W, D, -1)
        assert np.array_equal(out[:, :q], base[:, :q])
        assert np.array_equal(out[:, q, 0], base[:, q, 0])
        assert not np.array_equal(out[:, q, 1:], base[:, q, 1:])
        if q + 1 < H * W:
            assert not np.array_equal(out[:, q + 1:], base[:, q + 1:])
        for d in range(D):
            ch = codes.reshape(B, H * W, D).copy()
            ch[:, q, d] = (ch[:, q, d] + 7) % V                      # depth d of position q only
            out = eng.forward_onepass(T(ch.reshape(codes.shape)), T(cond), cbs).numpy().reshape(B, H * W, D, -1)
            assert np.array_equal(out[:, :q], base[:, :q])
            assert np.array_equal(out[:, q, :d + 1], base[:, q, :d + 1])
    perm = np.roll(np.arange(B), 1)
    out = eng.forward_onepass(T(codes[perm]), T(cond[perm]), cbs).numpy().reshape(B, H * W, D, -1)
    assert np.array_equal(out, base[perm])                           # permuting the images permutes the logits


# ---------------------------------------------------------------------------------------------- 4. log-probabilities
# log_prob_kernel against float64 log_softmax of the one-pass logits of the same call, gathered at the codes.
# Measured maximum on the emulator over rqt_tiny, rqt_tiny_txt (codes and conditioning tokens), the chunked and the depth-1 case:
# 5.74e-7 (log-probabilities of -4.9 .. -7.8, whose fp32 spacing is 4.8e-7: about one unit in the last place).  Bound = 2 x that.
LOGP_MEASURED = 5.74e-7
LOGP_BOUND = 2 * LOGP_MEASURED


def _logp64(logits, codes):
    x = logits.astype(np.float64)
    x = x - x.max(-1, keepdims=True)
    lsm = x - np.log(np.exp(x).sum(-1, keepdims=True))
    return np.take_along_axis(lsm, codes.reshape(lsm.shape[:-1] + (1,)), -1)[..., 0]


@needs_clang
def test_emu_log_probs(nat, golden):
    """log_probs against fp64 log_softmax (numpy) of the one-pass logits of the same inputs, gathered at the codes: measured
    maximum 5.74e-7 on the emulator, bound 1.148e-6 (LOGP_BOUND = 2 x the measured maximum)."""
    g, cfg, params, cb, eng = _tiny(nat, golden)
    codes, cond = g['codes'].astype(np.int64), g['cond'].astype(np.int64)
    logits = eng.forward_onepass(T(codes), T(cond), [T(cb)] * 4).numpy()
    lp = eng.log_probs(T(codes), T(cond), [T(cb)] * 4)
    assert lp.shape == codes.shape and lp.dtype == torch.float32
    e = np.abs(lp.numpy() - _logp64(logits, codes)).max()
    print('emu log_probs rqt_tiny: max err vs fp64 log_softmax %.3g' % e)
    assert e < LOGP_BOUND
    gt, cfgt, pt, cbt, engt = _tiny(nat, golden, 'rqt_tiny_txt.npz', C.RQT_TINY_TXT)
    codes, cond = gt['codes'].astype(np.int64), gt['cond'].astype(np.int64)
    seq, cl = engt.forward_onepass(T(codes), T(cond), [T(cbt)] * 4)
    lp, clp = engt.log_probs(T(codes), T(cond), [T(cbt)] * 4)
    assert clp.shape == (codes.shape[0], cfgt['block_size_cond'] - 1)
    e1 = np.abs(lp.numpy() - _logp64(seq.numpy(), codes)).max()
    e2 = np.abs(clp.numpy() - _logp64(cl.numpy(), cond[:, 1:])).max()
    print('emu log_probs rqt_tiny_txt: max err %.3g (codes) %.3g (cond)' % (e1, e2))
    assert e1 < LOGP_BOUND and e2 < LOGP_BOUND
    # a code outside the vocabulary has no probability
    bad = codes.copy()
    bad[0, 0, 0, 0] = cfgt['vocab_size']
    # (position 0 / depth 0 is never embedded for its own logit: only that one entry is NaN at depth 0; later ones see a padding row)
    lpb, _ = engt.log_probs(T(bad), T(cond), [T(cbt)] * 4)
    assert np.isnan(lpb.numpy()[0, 0, 0, 0])


@needs_clang
def test_emu_model_log_probs_and_losses(nat, golden):
    """RQTransformer.log_probs / compute_codebook_loss / compute_cond_loss over the mirror classes."""
    import torch.nn.functional as F
    g, ar, vae = _variant_model(golden, 'txtheads')
    codes, cond = T(g['codes'].astype(np.int64)), T(g['cond'].astype(np.int64))
    ar.forward_mode = 'one_pass'
    seq, cl = ar(codes, vae, cond=cond)
    lp, clp = ar.log_probs(codes, vae, cond=cond)
    assert abs(float(ar.compute_loss(seq, codes)) + float(lp.double().mean())) < 1e-5
    assert abs(float(ar.compute_cond_loss(cl, cond)) + float(clp.double().mean())) < 1e-5
    per = ar.compute_codebook_loss(seq, codes)
    want = F.cross_entropy(seq.reshape(-1, seq.shape[-1]), codes.reshape(-1), reduction='none').reshape(-1, codes.shape[-1]).mean(0)
    assert per.shape == (codes.shape[-1],) and torch.equal(per, want)
    assert torch.allclose(per, -lp.reshape(-1, codes.shape[-1]).mean(0), atol=1e-5)
    ar.forward_mode = 'sideways'
    with pytest.raises(ValueError):
        ar(codes, vae, cond=cond)


def test_forward_mode_default_and_env(monkeypatch):
    from rqvae.models.rqtransformer import RQTransformer
    monkeypatch.delenv('RQAMD_FORWARD', raising=False)
    assert RQTransformer(C.RQT_TINY).forward_mode == 'stepped'
    monkeypatch.setenv('RQAMD_FORWARD', 'one_pass')
    assert RQTransformer(C.RQT_TINY).forward_mode == 'one_pass'


# ---------------------------------------------------------------------------------------------- 4a. no scratch on gfx950
NEW_KERNELS = ('attn_prefill_kernel', 'attn_generic_prefill_kernel', 'attn_packed_kernel', 'gather_codes_kernel', 'body_input_kernel',
               'head_input_kernel', 'log_prob_kernel')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
@pytest.mark.parametrize('f16', [False, True])
def test_onepass_kernels_use_no_scratch(f16, tmp_path):
    """rqt_kernels.hip compiled for gfx950 with -Rpass-analysis=kernel-resource-usage: the attention (cache-free causal, packed
    short-sequence), gather and log-softmax kernels of the one-pass path keep everything in registers, in both builds."""
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-I', CSRC,
           '-Rpass-analysis=kernel-resource-usage', '--cuda-device-only', '-c', os.path.join(CSRC, 'rqt_kernels.hip'),
           '-o', str(tmp_path / 'k.o')] + (['-DRQ_F16=1'] if f16 else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    name = None
    for line in res.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
        m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', line)
        if m and name:
            seen[name] = int(m.group(1))
    mine = {k: v for k, v in seen.items() if any(n in k for n in NEW_KERNELS)}
    for n in NEW_KERNELS:
        assert any(n in k for k in mine), f'{n} not found in the resource-usage remarks'
    assert len([k for k in mine if 'attn_prefill_kernel' in k and 'generic' not in k]) == 2      # the appending and the cache-free form
    assert len([k for k in mine if 'attn_packed_kernel' in k]) == 3
    assert all(v == 0 for v in mine.values()), {k: v for k, v in mine.items() if v}


# ---------------------------------------------------------------------------------------------- 4b. argument checks
def test_onepass_status_codes_without_gpu():
    """the two entry points refuse bad arguments before any HIP call (observable on a GPU-less host), in both builds"""
    import ctypes
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from rqvae import _native
    for path in (_native.LIB_PATH, _native.LIB16_PATH):
        lib = ctypes.CDLL(path)
        lib.rqamd_last_error.restype = ctypes.c_char_p
        fake = ctypes.create_string_buffer(1 << 16)          # stands for a handle: the checks below return before reading it
        one = ctypes.c_void_p(8)                             # never dereferenced either
        for fn in (lib.rqamd_rqt_forward_onepass, lib.rqamd_rqt_log_probs):
            fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 4
            assert fn(None, one, None, 1, one, one, None, None) == -1           # null handle
            assert b'null' in lib.rqamd_last_error()
            assert fn(fake, None, None, 1, one, one, None, None) == -1          # null codes
            assert fn(fake, one, None, 1, None, one, None, None) == -1          # null codebooks
            assert fn(fake, one, None, 1, one, None, None, None) == -1          # null output
            assert b'null' in lib.rqamd_last_error()
            assert fn(fake, one, None, 0, one, one, None, None) == -1           # batch < 1
            assert b'batch < 1' in lib.rqamd_last_error()
        assert lib.rqamd_rqt_set_option(None, b'fwd.chunk_rows', 128) == -1
