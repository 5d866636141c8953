"""Body contexts beyond 256 tokens on the MI355X (`pytest -m gpu`): the chunked decode attention (attn_long_kernel), the tiled prefill /
cache-free attention (attn_prefill_tiled_kernel) and the engine's catch-all graph, through the mirror classes, against the reference's own
logits (fixtures rqt_long_txt300.npz / rqt_long_map.npz, tests/golden/make_golden_long.py).  Tiny widths (E 128, two heads of 64).

rqt_long_txt300: block_size (4, 4, 2) behind 300 text tokens -- P = 299 prefix tokens through the tiled prefill, decode steps t = 299 .. 314.
rqt_long_map: 32 x 32 x 2 behind 64 text tokens -- context 1087: decode steps t = 63 .. 1086 cross from the register kernels to the chunked
one at 256 keys, the one-pass forward runs 17 query tiles per (image, head)."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import configs as C

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import long_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# ceilings: the project's tiny-width bounds (tests/test_emu_kernels.py, tests/test_gpu_forward_onepass.py; same widths here)
REF_MAX, REF_MEAN = 0.06, 0.01          # bf16 engine against the reference
PATH_MAX = 0.02                         # stepped against one-pass, forced kernels against the default ones
F16_MAX, F16_MEAN = 0.004, 0.0006       # fp16 engine (amp=True) against the reference: tests/test_gpu_parity.py
# measured on the MI355X ("long contexts"): the bounds are at most twice these and never above the ceilings
MEASURED = {'logits': (0.0100, 0.00173), 'cond_logits': (0.0053, 0.00127), 'logp': (0.0069, 0.00180), 'paths': 0.00686, 'f16': (0.0012, 0.00022)}
B_LOGITS = (min(REF_MAX, 2 * MEASURED['logits'][0]), min(REF_MEAN, 2 * MEASURED['logits'][1]))
B_COND = (min(REF_MAX, 2 * MEASURED['cond_logits'][0]), min(REF_MEAN, 2 * MEASURED['cond_logits'][1]))
B_LOGP = (min(2 * REF_MAX, 2 * MEASURED['logp'][0]), min(2 * REF_MEAN, 2 * MEASURED['logp'][1]))      # twice the logits ceiling
B_PATHS = min(PATH_MAX, 2 * MEASURED['paths'])
B_F16 = (min(F16_MAX, 2 * MEASURED['f16'][0]), min(F16_MEAN, 2 * MEASURED['f16'][1]))


def G(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


class Aux:
    """minimal model_aux: only its codebook list is used by the engine"""

    def __init__(self, cb, depth):
        t = G(cb)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def _model(cfg, seed):
    from rqvae.models.rqtransformer import RQTransformer
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    ar = RQTransformer(cfg)
    ar.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqt_param_shapes(cfg), seed, cfg).items()}, strict=True)
    return ar.to(DEV).eval()


def _close(got, want, what, bound):
    err = np.abs(np.asarray(got, np.float64) - want)
    print('long context, %s: max err %.4f mean err %.5f' % (what, err.max(), err.mean()))
    assert err.max() < bound[0] and err.mean() < bound[1], what


def _logp(logits, targets):
    x = np.asarray(logits, np.float64)
    lse = np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1)) + x.max(-1)
    return np.take_along_axis(x, targets[..., None], -1)[..., 0] - lse


def _support(codes, logits, top_k, top_p, positions):
    """every drawn code has non-zero probability under the filtered distribution of the teacher-forced logits"""
    B, H, W, D = codes.shape
    for pos in positions:
        h, w = divmod(int(pos), W)
        for d in range(D):
            pr = oracle.filtered_probs(logits[:, h, w, d], 1.0, top_k, top_p)
            assert (pr[np.arange(B), codes[:, h, w, d]] > 0).all(), (h, w, d)


@pytest.fixture(scope='module')
def fixtures(golden):
    """(cfg, model, aux, codes, cond, reference dict) of the two fixtures, loaded once; the stored positions of both as flat indices"""
    out = {}
    for tag, cfg in (('txt300', L.txt_cfg(300, n_body=2)), ('map', L.map_cfg())):
        g = golden(f'rqt_long_{tag}.npz')
        cb, codes, cond = L.inputs(cfg, int(g['input_seed']))
        H, W, D = cfg['block_size']
        pos = np.arange(H * W) if tag == 'txt300' else g['pos']
        out[tag] = dict(cfg=cfg, ar=_model(cfg, int(g['seed'])), aux=Aux(cb, D), codes=G(codes, torch.long), cond=G(cond, torch.long),
                        pos=pos, logits=g['logits'].reshape(2, len(pos), D, -1), cond_pos=g['cond_pos'], cond_logits=g['cond_logits'],
                        codes_np=codes, cond_np=cond)
    yield out
    out.clear()
    torch.cuda.empty_cache()


def _at(t, pos):
    """(B, H, W, ...) -> (B, len(pos), ...) at flat spatial positions"""
    a = N(t)
    return a.reshape((a.shape[0], a.shape[1] * a.shape[2]) + a.shape[3:])[:, pos]


# ---------------------------------------------------------------------------------------------- 7. against the reference
@pytest.mark.parametrize('scale', [1, 4096])
@pytest.mark.parametrize('tag', ['txt300', 'map'])
def test_long_context_vs_reference(fixtures, tag, scale):
    """stepped forward, forward_mode = 'one_pass', log_probs and cond_logits at 2 images; once more under dbg_set_row_scale(4096), where
    the large-batch kernel choices run (one wavefront per pair in the chunked decode kernel, the large GEMM tiles)"""
    from rqvae import _native as nat
    f = fixtures[tag]
    ar, aux, codes, cond, pos = f['ar'], f['aux'], f['codes'], f['cond'], f['pos']
    what = f'{tag}, row scale {scale}'
    nat.dbg_set_row_scale(scale)
    try:
        ar.forward_mode = 'stepped'
        seq, cl = ar(codes, aux, cond=cond)
        ar.forward_mode = 'one_pass'
        seq1, cl1 = ar(codes, aux, cond=cond)
        lp, clp = ar.log_probs(codes, aux, cond=cond)
    finally:
        nat.dbg_set_row_scale(1)
        ar.forward_mode = 'stepped'
    _close(_at(seq, pos), f['logits'], what + ' stepped seq_logits', B_LOGITS)
    _close(N(cl)[:, f['cond_pos']], f['cond_logits'], what + ' stepped cond_logits', B_COND)
    _close(_at(seq1, pos), f['logits'], what + ' one-pass seq_logits', B_LOGITS)
    _close(N(cl1)[:, f['cond_pos']], f['cond_logits'], what + ' one-pass cond_logits', B_COND)
    d = max(float((seq1 - seq).abs().max()), float((cl1 - cl).abs().max()))
    print('long context, %s: stepped vs one-pass %.5f' % (what, d))
    assert d < B_PATHS
    tg = f['codes_np'].reshape(2, -1, f['codes_np'].shape[-1])[:, pos]
    _close(_at(lp, pos), _logp(f['logits'], tg), what + ' log_probs', B_LOGP)
    _close(N(clp)[:, f['cond_pos']], _logp(f['cond_logits'], f['cond_np'][:, 1:][:, f['cond_pos']]), what + ' cond log_probs', B_LOGP)


# ---------------------------------------------------------------------------------------------- 8. the fp16 build
def test_long_context_amp(fixtures):
    """amp=True on rqt_long_txt300: the fp16 build of the same kernels, stepped and one-pass, against the reference's fp32 logits"""
    f = fixtures['txt300']
    ar, aux, codes, cond = f['ar'], f['aux'], f['codes'], f['cond']
    seq, cl = ar(codes, aux, cond=cond, amp=True)
    _close(_at(seq, f['pos']), f['logits'], 'txt300 amp stepped seq_logits', B_F16)
    _close(N(cl)[:, f['cond_pos']], f['cond_logits'], 'txt300 amp stepped cond_logits', B_F16)
    ar.forward_mode = 'one_pass'
    try:
        seq1, cl1 = ar(codes, aux, cond=cond, amp=True)
    finally:
        ar.forward_mode = 'stepped'
    _close(_at(seq1, f['pos']), f['logits'], 'txt300 amp one-pass seq_logits', B_F16)
    _close(N(cl1)[:, f['cond_pos']], f['cond_logits'], 'txt300 amp one-pass cond_logits', B_F16)


# ---------------------------------------------------------------------------------------------- 9. sampling behind 300 text tokens
def test_long_context_sample_txt300():
    """C = 300, 4 images: graph == eager and cached == uncached bit for bit (positions t >= 256 all replay the catch-all graph);
    cached_forward stepped in sampling order == forward bit for bit; every draw inside the support of the teacher-forced logits; the attention
    profile of the engine counts the chunked kernel's launches"""
    cfg = L.txt_cfg(300, n_body=2)
    ar = _model(cfg, L.TXT300_SEED)
    cb, _, cond = L.inputs(cfg, 81, n_img=4)
    aux, cond = Aux(cb, 2), G(cond, torch.long)
    partial = torch.zeros((4, 4, 4, 2), dtype=torch.long, device=DEV)
    res = []
    for graph, cached in ((True, True), (False, True), (True, False)):
        ar.use_graph = graph
        torch.cuda.manual_seed_all(5)
        res.append(ar.sample(partial, aux, cond=cond, top_k=5, top_p=0.9, cached=cached))
    ar.use_graph = True
    assert torch.equal(res[0], res[1]), 'graph != eager'
    assert torch.equal(res[0], res[2]), 'cached != uncached'
    codes = res[0]
    assert int(codes.min()) >= 0 and int(codes.max()) < 500
    full, _ = ar(codes, aux, cond=cond)
    _support(N(codes), N(full), 5, 0.9, range(16))
    ar.init_cache()
    for h in range(4):
        for w in range(4):
            for d in range(2):
                lg = ar.cached_forward(codes[:, :h + 1], aux, cond=cond, sample_loc=(h, w, d))
                assert torch.equal(lg, full[:, h, w, d]), (h, w, d)
    ar.init_cache()
    # rqamd_rqt_get_profile_attn brackets the chunked kernel's launches like the others: 16 positions x (2 body + 2 depths x 1 head layer)
    eng = ar._eng()
    eng.set_profile(True)
    try:
        torch.cuda.manual_seed_all(5)
        prof_codes = ar.sample(partial, aux, cond=cond, top_k=5, top_p=0.9)
        torch.cuda.synchronize()
        pf = eng.get_profile()
    finally:
        eng.set_profile(False)
    assert torch.equal(prof_codes, codes)
    assert pf['attn_launches'] == 16 * (2 + 2 * 1) and pf['attn_ms_total'] > 0, pf


# ---------------------------------------------------------------------------------------------- 10. sampling a 32 x 32 map
def test_long_context_sample_map(fixtures, golden):
    """32 x 32 x 2 behind 64 text tokens, 2 images, with graphs: 24 bucket graphs, then the catch-all graph for the 831 positions from token
    256 on.  Codes in range, inside the support at the fixture's stored positions, the same codes for the same seed -- and a short-context
    module sampled before and after gives unchanged codes (its graphs and workspace are its own)."""
    from rqvae.models.rqvae import RQVAE
    gt = golden('rqt_tiny.npz')
    hps, dd = C.VAE_TINY
    vae = RQVAE(**hps, ddconfig=dd, checkpointing=False)
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqvae_param_shapes(hps, dd), int(gt['vae_seed'])).items()})
    vae = vae.to(DEV).eval()
    tiny = _model(C.RQT_TINY, int(gt['seed']))
    tcond = G(gt['cond'], torch.long)[:2].contiguous()
    tpart = torch.zeros((2, 4, 4, 4), dtype=torch.long, device=DEV)
    torch.cuda.manual_seed_all(9)
    before = tiny.sample(tpart, vae, cond=tcond, top_k=20, top_p=0.9)

    f = fixtures['map']
    ar, aux, cond = f['ar'], f['aux'], f['cond']
    partial = torch.zeros((2, 32, 32, 2), dtype=torch.long, device=DEV)
    assert ar.use_graph
    torch.cuda.manual_seed_all(7)
    codes = ar.sample(partial, aux, cond=cond, top_k=5, top_p=0.9)
    assert codes.shape == partial.shape and int(codes.min()) >= 0 and int(codes.max()) < 500
    torch.cuda.manual_seed_all(7)
    assert torch.equal(ar.sample(partial, aux, cond=cond, top_k=5, top_p=0.9), codes)
    full, _ = ar(codes, aux, cond=cond)
    _support(N(codes), N(full), 5, 0.9, f['pos'])

    torch.cuda.manual_seed_all(9)
    assert torch.equal(tiny.sample(tpart, vae, cond=tcond, top_k=20, top_p=0.9), before)


# ---------------------------------------------------------------------------------------------- 11. the new kernels on today's fixtures
def test_forced_kernels_on_short_contexts(golden, monkeypatch):
    """RQAMD_PREFILL_TILED=1 / RQAMD_ATTN_LONG=1 on rqt_tiny_txt and on the 70-token prefix of the emulator tests.  The tiled prefill keeps
    the per-query key order and recurrence of attn_prefill_kernel: bit-identical, stepped and one-pass.  The chunked decode kernel: within the
    reference bound and within 0.02 of the register kernels."""
    hps, dd = C.VAE_TINY
    g = golden('rqt_tiny_txt.npz')
    cbt = oracle.make_params(oracle.rqvae_param_shapes(hps, dd), int(g['vae_seed']))['quantizer.codebooks.0.weight'][:-1]
    cfgl = C.rqt(128, 2, 1, 1, 500, vocab_cond=20, block_cond=70, block_size=(4, 4, 4), input_embed_dim=64)
    rng = np.random.default_rng(44)
    cbl = rng.standard_normal((500, 64), dtype=np.float32)
    codes_l, cond_l = rng.integers(0, 500, (2, 4, 4, 4)), rng.integers(0, 20, (2, 70))
    ref_l = oracle.RQTransformerOracle(cfgl, oracle.make_params(oracle.rqt_param_shapes(cfgl), 43)).forward(codes_l, [cbl] * 4, cond_l)
    cases = [('rqt_tiny_txt', _model(C.RQT_TINY_TXT, int(g['seed'])), cbt, g['codes'].astype(np.int64), g['cond'].astype(np.int64), g['logits']),
             ('prefix70', _model(cfgl, 43), cbl, codes_l, cond_l, ref_l)]
    for tag, ar, cb, codes, cond, ref in cases:
        aux, codes, cond = Aux(cb, 4), G(codes, torch.long), G(cond, torch.long)

        def both():
            ar.forward_mode = 'stepped'
            a = ar(codes, aux, cond=cond)
            ar.forward_mode = 'one_pass'
            b = ar(codes, aux, cond=cond)
            ar.forward_mode = 'stepped'
            return a + b
        base = both()
        monkeypatch.setenv('RQAMD_PREFILL_TILED', '1')
        tiled = both()
        monkeypatch.delenv('RQAMD_PREFILL_TILED')
        assert all(torch.equal(x, y) for x, y in zip(tiled, base)), tag
        monkeypatch.setenv('RQAMD_ATTN_LONG', '1')
        seq_l, cl_l = ar(codes, aux, cond=cond)
        monkeypatch.delenv('RQAMD_ATTN_LONG')
        err = np.abs(N(seq_l) - ref)
        d = float((seq_l - base[0]).abs().max())
        print('forced chunked decode on %s: max err %.4f mean %.5f, vs the register kernels %.5f' % (tag, err.max(), err.mean(), d))
        assert err.max() < REF_MAX and err.mean() < REF_MEAN
        assert d < PATH_MAX
        assert torch.equal(cl_l, base[1])
