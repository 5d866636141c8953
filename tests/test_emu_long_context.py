"""CPU-only checks of body contexts beyond 256 tokens (attn_long_kernel, attn_prefill_tiled_kernel, the engine's catch-all position)
through the host emulator (tests/emu): the same .hip sources executed by fibers, against the numpy oracle (valid at these lengths:
tests/golden/make_golden_long.py prints oracle vs reference, 1.7e-6) and the reference-generated fixture rqt_long_txt300.npz.
The authoritative runs are the `-m gpu` ones (tests/test_gpu_long_context.py).  Neither new kernel uses LDS-DMA, so RQ_EMU_DMA has
nothing to vary here.

A long text prefix makes a long context without many steps: block_size (4, 4, 2) behind C conditioning tokens is a context of 15 + C with
16 stepped positions; the prefix is P = C - 1 tokens, position pos attends over keys 0 .. t with t = pos + C - 1.  Two (row, head) pairs
per image and two images: the decode kernel runs its four-wavefronts-per-pair form, and its one-wavefront form under dbg_set_row_scale."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import configs as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import long_cases as L  # noqa: E402

CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')

# ceilings: the project's tiny-width bounds (tests/test_emu_kernels.py, tests/test_gpu_forward_onepass.py; same widths here)
REF_MAX, REF_MEAN = 0.06, 0.01          # logits against the reference / the oracle
PATH_MAX = 0.02                         # stepped against one-pass, forced kernels against the default ones
# measured ("long contexts"): the bounds below are at most twice these and never above the ceilings
MEASURED = {'logits': (0.0104, 0.00177), 'cond_logits': (0.0069, 0.00127), 'logp': (0.0062, 0.00177), 'paths': 0.00327}
B_LOGITS = (min(REF_MAX, 2 * MEASURED['logits'][0]), min(REF_MEAN, 2 * MEASURED['logits'][1]))
B_COND = (min(REF_MAX, 2 * MEASURED['cond_logits'][0]), min(REF_MEAN, 2 * MEASURED['cond_logits'][1]))
B_LOGP = (min(2 * REF_MAX, 2 * MEASURED['logp'][0]), min(2 * REF_MEAN, 2 * MEASURED['logp'][1]))      # log-probabilities: twice the logits ceiling
B_PATHS = min(PATH_MAX, 2 * MEASURED['paths'])


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


def _engine(nat, cfg, params):
    eng = nat.RqtEngine(embed_dim=cfg['embed_dim'], n_head=cfg['body']['block']['n_head'], n_layer_body=cfg['body']['n_layer'],
                        n_layer_head=cfg['head']['n_layer'], vocab_size=cfg['vocab_size'], input_embed_dim=cfg['input_embed_dim'],
                        vocab_size_cond=cfg['vocab_size_cond'], block_size_cond=cfg['block_size_cond'],
                        block_size=cfg['block_size'], gelu_v2=cfg.get('gelu', 'v1') == 'v2', device='cpu')
    for k, v in params.items():
        eng.set_param(k, T(v))
    return eng


def _close(got, want, what, bound):
    err = np.abs(np.asarray(got, np.float64) - want)
    print('emu long context, %s: max err %.4f mean err %.5f' % (what, err.max(), err.mean()))
    assert err.max() < bound[0] and err.mean() < bound[1], what


def _logp(logits, targets):
    x = np.asarray(logits, np.float64)
    lse = np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1)) + x.max(-1)
    return np.take_along_axis(x, targets[..., None], -1)[..., 0] - lse


_ORACLE = {}


def _case(block_cond, n_body=1, seed=51):
    """(cfg, params, cb, codes, cond, oracle seq_logits, oracle cond_logits) -- computed once per shape, shared, never written to"""
    key = (block_cond, n_body, seed)
    if key not in _ORACLE:
        cfg = L.txt_cfg(block_cond, n_body)
        params = oracle.make_params(oracle.rqt_param_shapes(cfg), seed)
        cb, codes, cond = L.inputs(cfg, seed + 1)
        ref = oracle.RQTransformerOracle(cfg, params).forward(codes, [cb] * 2, cond, return_cond_logits=True)
        _ORACLE[key] = (cfg, params, cb, codes, cond, ref[0], ref[1])
    return _ORACLE[key]


def _all_paths(eng, cb, codes, cond, seq_ref, cl_ref, tag):
    """stepped logits, forward with cond_logits, forward_onepass and log_probs of one engine against one reference"""
    cbs = [T(cb)] * 2
    seq, cl = eng.forward(T(codes), T(cond), cbs)      # (rqamd_rqt_logits is the same stepping without cond_logits: test_emu_long_context_sample)
    _close(seq.numpy(), seq_ref, tag + ' stepped seq_logits', B_LOGITS)
    _close(cl.numpy(), cl_ref, tag + ' stepped cond_logits', B_COND)
    seq1, cl1 = eng.forward_onepass(T(codes), T(cond), cbs)
    _close(seq1.numpy(), seq_ref, tag + ' one-pass seq_logits', B_LOGITS)
    _close(cl1.numpy(), cl_ref, tag + ' one-pass cond_logits', B_COND)
    d = max(np.abs(seq1.numpy() - seq.numpy()).max(), np.abs(cl1.numpy() - cl.numpy()).max())
    print('emu long context, %s: stepped vs one-pass %.5f' % (tag, d))
    assert d < B_PATHS
    lp, clp = eng.log_probs(T(codes), T(cond), cbs)
    _close(lp.numpy(), _logp(seq_ref, codes), tag + ' log_probs', B_LOGP)
    _close(clp.numpy(), _logp(cl_ref, cond[:, 1:]), tag + ' cond log_probs', B_LOGP)
    return seq.numpy(), cl.numpy()


# ---------------------------------------------------------------------------------------------- 1. across the 256-token boundary
@pytest.mark.parametrize('block_cond', [250, 300])
def test_emu_long_context_paths(nat, block_cond):
    """C = 250: P = 249 keeps the one-wavefront prefill, the decode steps cross 256 keys (t = 249 .. 264: register kernel, then the chunked
    one).  C = 300: P = 299 runs the tiled prefill, every decode step the chunked kernel (t = 299 .. 314).  One body layer each."""
    cfg, params, cb, codes, cond, seq_ref, cl_ref = _case(block_cond)
    eng = _engine(nat, cfg, params)
    seq, cl = _all_paths(eng, cb, codes, cond, seq_ref, cl_ref, f'C={block_cond}')
    nat.dbg_set_row_scale(4096)          # the large-batch kernel choices: one wavefront per pair in the chunked decode kernel
    try:
        big, clb = eng.forward(T(codes), T(cond), [T(cb)] * 2)
    finally:
        nat.dbg_set_row_scale(1)
    _close(big.numpy(), seq_ref, f'C={block_cond} large-batch kernel variants', B_LOGITS)
    d = max(np.abs(big.numpy() - seq).max(), np.abs(clb.numpy() - cl).max())
    print('emu long context, C=%d: large-batch vs small-batch kernel variants %.5f' % (block_cond, d))
    assert d < B_PATHS


def test_emu_long_context_txt300_fixture(nat, golden):
    """rqt_long_txt300.npz: the reference's own logits (two body layers, C = 300) at every position, cond_logits at the stored prefix positions"""
    g = golden('rqt_long_txt300.npz')
    cfg = L.txt_cfg(300, n_body=2)
    params = oracle.make_params(oracle.rqt_param_shapes(cfg), int(g['seed']))
    cb, codes, cond = L.inputs(cfg, int(g['input_seed']))
    eng = _engine(nat, cfg, params)
    seq, cl = eng.forward(T(codes), T(cond), [T(cb)] * 2)
    _close(seq.numpy(), g['logits'], 'txt300 fixture stepped seq_logits', B_LOGITS)
    _close(cl.numpy()[:, g['cond_pos']], g['cond_logits'], 'txt300 fixture stepped cond_logits', B_COND)
    seq1, cl1 = eng.forward_onepass(T(codes), T(cond), [T(cb)] * 2)
    _close(seq1.numpy(), g['logits'], 'txt300 fixture one-pass seq_logits', B_LOGITS)
    _close(cl1.numpy()[:, g['cond_pos']], g['cond_logits'], 'txt300 fixture one-pass cond_logits', B_COND)
    assert np.abs(seq1.numpy() - seq.numpy()).max() < B_PATHS


# ---------------------------------------------------------------------------------------------- 2. the kernels' internal boundaries
@pytest.mark.parametrize('block_cond', [320, 321, 322])
def test_emu_long_context_chunk_and_tile_edges_stepped(nat, block_cond):
    """Register chunks of the decode kernel and key / query tiles of the tiled prefill are 64 keys, so 320 = 5 * 64 is an edge of both.
    C = 320: P = 319 ends one key before the tile edge; the decode steps t = 319 .. 334 end one key before the chunk edge (t = 319 fills
    chunk 4), on it (t = 320: chunk 5 holds one key, which is this token's own) and after it, with lengths that are no multiple of 8.
    C = 321: P = 320 fills five tiles exactly.  C = 322: P = 321 leaves one query (and one key) in the sixth tile."""
    cfg, params, cb, codes, cond, seq_ref, cl_ref = _case(block_cond)
    eng = _engine(nat, cfg, params)
    seq, cl = eng.forward(T(codes), T(cond), [T(cb)] * 2)
    _close(seq.numpy(), seq_ref, f'C={block_cond} stepped seq_logits', B_LOGITS)
    _close(cl.numpy(), cl_ref, f'C={block_cond} stepped cond_logits', B_COND)


@pytest.mark.parametrize('block_cond', [304, 305, 306])
def test_emu_long_context_tile_edges_onepass(nat, block_cond):
    """the cache-free form of the tiled attention over all 15 + C body tokens: 319 (one before the tile edge), 320 (five full tiles) and
    321 (one query in the sixth tile)"""
    cfg, params, cb, codes, cond, seq_ref, cl_ref = _case(block_cond)
    eng = _engine(nat, cfg, params)
    seq, cl = eng.forward_onepass(T(codes), T(cond), [T(cb)] * 2)
    _close(seq.numpy(), seq_ref, f'C={block_cond} one-pass seq_logits', B_LOGITS)
    _close(cl.numpy(), cl_ref, f'C={block_cond} one-pass cond_logits', B_COND)


# ---------------------------------------------------------------------------------------------- 3. the new kernels on today's fixtures
def _short_cases(golden):
    g = golden('rqt_tiny_txt.npz')
    cfg = C.RQT_TINY_TXT
    hps, dd = C.VAE_TINY
    cbt = oracle.make_params(oracle.rqvae_param_shapes(hps, dd), int(g['vae_seed']))['quantizer.codebooks.0.weight'][:-1]
    pt = oracle.make_params(oracle.rqt_param_shapes(cfg), int(g['seed']))
    codes, cond = g['codes'].astype(np.int64), g['cond'].astype(np.int64)
    ref = oracle.RQTransformerOracle(cfg, pt).forward(codes, [cbt] * 4, cond, return_cond_logits=True)
    yield 'rqt_tiny_txt', cfg, pt, cbt, codes, cond, g['logits'], ref[1]
    # the 70-token prefix of test_emu_rqt_long_prefix
    cfg = C.rqt(128, 2, 1, 1, 500, vocab_cond=20, block_cond=70, block_size=(4, 4, 4), input_embed_dim=64)
    pl = oracle.make_params(oracle.rqt_param_shapes(cfg), 43)
    rng = np.random.default_rng(44)
    cbl = rng.standard_normal((500, 64), dtype=np.float32)
    codes, cond = rng.integers(0, 500, (2, 4, 4, 4)), rng.integers(0, 20, (2, 70))
    ref = oracle.RQTransformerOracle(cfg, pl).forward(codes, [cbl] * 4, cond, return_cond_logits=True)
    yield 'prefix70', cfg, pl, cbl, codes, cond, ref[0], ref[1]


def test_emu_forced_kernels_on_short_contexts(nat, golden, monkeypatch):
    """RQAMD_PREFILL_TILED=1: the tiled prefill keeps the per-query key order and recurrence of attn_prefill_kernel -- bit-identical, stepped
    and one-pass.  RQAMD_ATTN_LONG=1: contexts of more than 8 keys through the chunked decode kernel -- within the reference bound and within
    0.02 of the register kernels (another summation order; the bf16 rounding of the attention output hides it at most elements, so the two often
    agree to the bit and no difference is asserted).  The contexts here are 4 .. 19 and 70 .. 85 keys: one and two
    chunks, i.e. three and two of a pair's four wavefronts have no chunk at all."""
    for tag, cfg, params, cb, codes, cond, seq_ref, cl_ref in _short_cases(golden):
        cbs = [T(cb)] * 4
        eng = _engine(nat, cfg, params)
        seq, cl = eng.forward(T(codes), T(cond), cbs)
        seq1, cl1 = eng.forward_onepass(T(codes), T(cond), cbs)
        monkeypatch.setenv('RQAMD_PREFILL_TILED', '1')
        seq_t, cl_t = eng.forward(T(codes), T(cond), cbs)
        seq1_t, cl1_t = eng.forward_onepass(T(codes), T(cond), cbs)
        monkeypatch.delenv('RQAMD_PREFILL_TILED')
        assert torch.equal(seq_t, seq) and torch.equal(cl_t, cl), tag
        assert torch.equal(seq1_t, seq1) and torch.equal(cl1_t, cl1), tag
        for scale in (1, 4096):          # four wavefronts per pair / one (and, at 4096, the large-batch GEMM tiles on both sides of the bound)
            monkeypatch.setenv('RQAMD_ATTN_LONG', '1')
            nat.dbg_set_row_scale(scale)
            try:
                seq_l, cl_l = eng.forward(T(codes), T(cond), cbs)
            finally:
                nat.dbg_set_row_scale(1)
                monkeypatch.delenv('RQAMD_ATTN_LONG')
            err = np.abs(seq_l.numpy() - seq_ref)
            d = np.abs(seq_l.numpy() - seq.numpy()).max()
            print('emu forced chunked decode on %s (row scale %d): max err %.4f mean %.5f, vs the register kernels %.5f' % (tag, scale, err.max(), err.mean(), d))
            assert err.max() < REF_MAX and err.mean() < REF_MEAN
            assert d < PATH_MAX
            if scale == 1:
                assert torch.equal(cl_l, cl)                     # the prefix never sees a decode kernel


# ---------------------------------------------------------------------------------------------- 5. sampling
def test_emu_long_context_sample(nat):
    """sample(use_graph=False) at C = 250: every draw has non-zero probability under the filtered distribution of the engine's own teacher-
    forced logits (top-k 5, top-p 0.9)"""
    cfg, params, cb, codes, cond, _, _ = _case(250)
    eng = _engine(nat, cfg, params)
    cbs = [T(cb)] * 2
    out = eng.sample(torch.zeros((2, 4, 4, 2), dtype=torch.int64), T(cond), cbs, (0, 0), 1.0, [5] * 2, [0.9] * 2, seed=11, offset=0, use_graph=False)
    assert out.shape == (2, 4, 4, 2) and int(out.min()) >= 0 and int(out.max()) < 500
    tf = eng.logits(out, T(cond), cbs).numpy()
    for h in range(4):
        for w in range(4):
            for d in range(2):
                pr = oracle.filtered_probs(tf[:, h, w, d], 1.0, 5, 0.9)
                assert (pr[np.arange(2), out[:, h, w, d].numpy()] > 0).all()


# ---------------------------------------------------------------------------------------------- 6. what stays refused
def _create(nat, cfg):
    return nat.RqtEngine(embed_dim=cfg['embed_dim'], n_head=cfg['body']['block']['n_head'], n_layer_body=1, n_layer_head=1,
                         vocab_size=cfg['vocab_size'], input_embed_dim=cfg['input_embed_dim'], vocab_size_cond=cfg['vocab_size_cond'],
                         block_size_cond=cfg['block_size_cond'], block_size=cfg['block_size'], device='cpu')


def test_emu_long_context_refusals(nat, monkeypatch):
    """at creation, with a message that says why: context > RQT_MAX_CONTEXT; context > 256 with an 8-bit cache format; context > 256 with a head
    size other than 64.  A context of exactly RQT_MAX_CONTEXT is accepted."""
    assert nat.RQT_MAX_CONTEXT == 1088
    ok = C.rqt(128, 2, 1, 1, 500, vocab_cond=20, block_cond=65, block_size=(32, 32, 2), input_embed_dim=64)        # 1024 + 64
    _create(nat, ok).close()
    with pytest.raises(NotImplementedError, match='1089 > RQAMD_RQT_MAX_CONTEXT = 1088'):
        _create(nat, C.rqt(128, 2, 1, 1, 500, vocab_cond=20, block_cond=66, block_size=(32, 32, 2), input_embed_dim=64))
    with pytest.raises(NotImplementedError, match='context 257 > 256 needs head size 64'):
        _create(nat, C.rqt(128, 4, 1, 1, 500, vocab_cond=20, block_cond=242, block_size=(4, 4, 2), input_embed_dim=64))
    _create(nat, C.rqt(128, 4, 1, 1, 500, vocab_cond=20, block_cond=241, block_size=(4, 4, 2), input_embed_dim=64)).close()    # 256: the plain kernels
    for fmt in ('int8k', 'int8kv'):
        monkeypatch.setenv('RQAMD_KV', fmt)
        with pytest.raises(NotImplementedError, match='context 257 > 256 with RQAMD_KV=' + fmt):
            _create(nat, L.txt_cfg(242))
        _create(nat, L.txt_cfg(241)).close()
    monkeypatch.delenv('RQAMD_KV')
    # the one-pass forward refuses a row budget that holds no image instead of exceeding it
    cfg, params, cb, codes, cond, _, _ = _case(250)
    eng = _engine(nat, cfg, params)
    eng.set_option('fwd.chunk_rows', 264)
    with pytest.raises(ValueError, match='holds no image'):
        eng.forward_onepass(T(codes), T(cond), [T(cb)] * 2)
    eng.set_option('fwd.chunk_rows', 265)
    eng.forward_onepass(T(codes), T(cond), [T(cb)] * 2)
