"""The one-pass teacher-forced forward (forward_mode='one_pass', RQTransformer.log_probs) on the GPU: against logits produced by the
REFERENCE itself (tests/golden/make_golden.py rqt_big: fp32 on CPU, seeded weights) with the bounds tests/test_gpu_parity_big.py
applies to the stepped path -- the error must not depend on which GEMM kernel produced the logits -- and the new kernels against
float64.  Run with -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import configs as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

MAX_ERR, MEAN_ERR = 0.03, 0.0045                  # tests/test_gpu_parity_big.py, unchanged
# If every logit is within e of the reference's, a log-probability is within 2e (the target logit and the logsumexp each move by at
# most e): twice the bounds above -- derived, not measured.
LOGP_MAX_ERR, LOGP_MEAN_ERR = 0.06, 0.009
# log_prob_kernel alone, against float64 log_softmax of the one-pass logits of the same inputs: 2 x the maximum measured on the MI355X
# (test_log_probs_vs_float64's docstring)
LOGP_F64_MEASURED = 1.58e-6
LOGP_F64_BOUND = 2 * LOGP_F64_MEASURED


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


def _load(cfg, seed):
    from rqvae.models.rqtransformer import RQTransformer
    ar = RQTransformer(cfg)
    shapes = oracle.rqt_param_shapes(cfg)
    sd = ar.state_dict()
    with torch.no_grad():
        for k, shp in shapes.items():           # tensor by tensor: the 1.4B fp32 set is 5.5 GB
            sd[k].copy_(torch.from_numpy(oracle.weights.make_tensor(k, shp, seed)))
    return ar.to(DEV).eval()


def _case(golden, tag, cfg):
    g = golden(f'rqt_{tag}.npz')
    V, D = cfg['vocab_size'], cfg['block_size'][2]
    cb = np.random.default_rng(int(g['cb_seed'])).standard_normal((V, 256), dtype=np.float32)
    return g, Aux(cb, D), G(g['codes'], torch.long), G(g['cond'], torch.long)


@pytest.fixture(scope='module')
def big(golden):
    """the full ImageNet 1.4B model, loaded once"""
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()
    cfg = C.RQT_IN_1400M
    g, aux, codes, cond = _case(golden, 'in1400m', cfg)
    ar = _load(cfg, int(g['seed']))
    yield ar, cfg, g, aux, codes, cond
    del ar
    torch.cuda.empty_cache()


def _stored(out, g, r0=0):
    return N(torch.stack([out[r0:r0 + 2, int(h), int(w)] for h, w in g['pos']], 1))


def _check_logits(got, ref, what, max_err=MAX_ERR, mean_err=MEAN_ERR):
    err = np.abs(got - ref)
    print(f'one-pass {what}: logits max err {err.max():.4f} mean {err.mean():.5f}')
    assert err.max() < max_err and err.mean() < mean_err, what
    top2 = np.sort(ref, -1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 0.3
    if clear.any():
        assert (got.argmax(-1) == ref.argmax(-1))[clear].all(), what


def _logp64(logits, codes):
    x = logits.astype(np.float64)
    x = x - x.max(-1, keepdims=True)
    lsm = x - np.log(np.exp(x).sum(-1, keepdims=True))
    return np.take_along_axis(lsm, codes.reshape(lsm.shape[:-1] + (1,)), -1)[..., 0]


def _check_logp_vs_reference(lp, g, codes, what):
    """log_softmax(fixture logits)[codes] at the fixture's stored positions"""
    pos = g['pos']
    got = N(torch.stack([lp[:, int(h), int(w)] for h, w in pos], 1))                         # (B, n_pos, D)
    tg = N(torch.stack([codes[:, int(h), int(w)] for h, w in pos], 1))
    want = _logp64(g['logits'].astype(np.float32), tg)
    err = np.abs(got - want)
    print(f'one-pass {what}: log-probabilities max err {err.max():.4f} mean {err.mean():.5f} vs the reference')
    assert err.max() < LOGP_MAX_ERR and err.mean() < LOGP_MEAN_ERR, what


# ---------------------------------------------------------------------------------------------- 5, 6, 7, 10: the reference's logits
def test_onepass_in1400m_vs_reference(big, golden):
    ar, cfg, g, aux, codes, cond = big
    ref = g['logits'].astype(np.float32)
    ar.forward_mode = 'one_pass'
    try:
        out = ar(codes, aux, cond=cond)
        assert out.shape == (2, 8, 8, 4, cfg['vocab_size']) and out.dtype == torch.float32
        _check_logits(_stored(out, g), ref, 'in1400m, 2 images')
        # 64 images (the two fixture images tiled): 4096 body rows, 16384 head rows -- the large-batch GEMM families, four head sub-chunks
        codes64, cond64 = codes.repeat(32, 1, 1, 1), cond.repeat(32, 1)
        out64 = ar(codes64, aux, cond=cond64)
        for r0 in (0, 32, 62):
            _check_logits(_stored(out64, g, r0), ref, f'in1400m, 64 images, rows {r0}..{r0 + 1}')
        del out64
        # amp=True: the fp16 build -- the tightest check of the new attention kernels' arithmetic (bounds of test_rqt_in1400m_amp_fp16_engine)
        out16 = ar(codes, aux, cond=cond, amp=True)
        _check_logits(_stored(out16, g), ref, 'in1400m, fp16 engine, 2 images', 0.004, 0.0006)
        out16 = ar(codes64, aux, cond=cond64, amp=True)
        for r0 in (0, 32, 62):
            _check_logits(_stored(out16, g, r0), ref, f'in1400m, fp16 engine, 64 images, rows {r0}..{r0 + 1}', 0.004, 0.0006)
        del out16
    finally:
        ar.forward_mode = 'stepped'
    _check_logp_vs_reference(ar.log_probs(codes, aux, cond=cond), g, codes, 'in1400m')


@pytest.mark.parametrize('tag,cfg', [('ffhq355m', C.RQT_FFHQ_355M), ('xwide', C.RQT_XWIDE), ('txt32', C.RQT_TXT32), ('txt64', C.RQT_TXT64)])
def test_onepass_other_widths_vs_reference(golden, tag, cfg):
    from rqvae import _native
    _native.lib()
    g, aux, codes, cond = _case(golden, tag, cfg)
    ar = _load(cfg, int(g['seed']))
    ar.forward_mode = 'one_pass'
    out = ar(codes, aux, cond=cond)
    cond_logits = None
    if cfg['block_size_cond'] > 1:
        assert isinstance(out, tuple) and len(out) == 2
        out, cond_logits = out
    _check_logits(_stored(out, g), g['logits'].astype(np.float32), tag)
    if cond_logits is not None:
        assert cond_logits.shape == (codes.shape[0], cfg['block_size_cond'] - 1, cfg['vocab_size_cond'])
        cpos = torch.from_numpy(g['cond_pos'].astype(np.int64)).to(DEV)
        cref = g['cond_logits'].astype(np.float32)
        cerr = np.abs(N(cond_logits[:, cpos]) - cref)
        print(f'one-pass {tag}: cond_logits max err {cerr.max():.4f} mean {cerr.mean():.5f}')
        assert cerr.max() < MAX_ERR and cerr.mean() < MEAN_ERR
    if tag in ('ffhq355m', 'txt64'):
        lp = ar.log_probs(codes, aux, cond=cond)
        if cond_logits is not None:
            lp, clp = lp
            assert clp.shape == (codes.shape[0], cfg['block_size_cond'] - 1)
            # target of row t is cond[t + 1]
            want = _logp64(cref, N(cond[:, 1:][:, cpos]))
            e = np.abs(N(clp[:, cpos]) - want)
            print(f'one-pass {tag}: cond log-probabilities max err {e.max():.4f} mean {e.mean():.5f} vs the reference')
            assert e.max() < LOGP_MAX_ERR and e.mean() < LOGP_MEAN_ERR
        _check_logp_vs_reference(lp, g, codes, tag)
    del ar
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 8, 9: the tiny models
def _tiny_models(golden, name, cfg):
    from rqvae.models.rqvae import RQVAE
    from rqvae.models.rqtransformer import RQTransformer
    g = golden(name)
    hps, dd = C.VAE_TINY
    vae = RQVAE(**hps, ddconfig=dd, checkpointing=False)
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqvae_param_shapes(hps, dd), int(g['vae_seed'])).items()})
    ar = RQTransformer(cfg)
    ar.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqt_param_shapes(cfg), int(g['seed']), cfg).items()}, strict=True)
    return g, vae.to(DEV).eval(), ar.to(DEV).eval()


TINY = [('rqt_tiny.npz', 'RQT_TINY'), ('rqt_tiny_txt.npz', 'RQT_TINY_TXT'), ('rqt_var_tuple.npz', 'RQT_TINY_TUPLE'),
        ('rqt_var_nocumsum.npz', 'RQT_TINY_NOCUMSUM'), ('rqt_var_mixed.npz', 'RQT_TINY_MIXED'), ('rqt_var_nobias.npz', 'RQT_TINY_NOBIAS'),
        ('rqt_var_gelumix.npz', 'RQT_TINY_GELUMIX'), ('rqt_var_heads.npz', 'RQT_TINY_HEADS'), ('rqt_var_txtheads.npz', 'RQT_TINY_TXT_HEADS')]


@pytest.mark.parametrize('name,cfgname', TINY)
def test_onepass_tiny_and_flag_variants(golden, name, cfgname):
    g, vae, ar = _tiny_models(golden, name, getattr(C, cfgname))
    aux = vae if cfgname != 'RQT_TINY_TUPLE' else None
    codes, cond = G(g['codes'], torch.long), G(g['cond'], torch.long)
    ar.forward_mode = 'one_pass'
    out = ar(codes, aux, cond=cond)
    out = out[0] if isinstance(out, tuple) else out
    err = np.abs(N(out) - g['logits'])
    print(f'one-pass {name}: logits max err {err.max():.4f} mean {err.mean():.5f}')
    assert err.max() < 0.06 and err.mean() < 0.01
    assert torch.equal(ar.teacher_forced_logits(codes, aux, cond=cond), out)
    lp = ar.log_probs(codes, aux, cond=cond)
    lp = lp[0] if isinstance(lp, tuple) else lp
    assert np.abs(N(lp) - _logp64(N(out), N(codes))).max() < LOGP_F64_BOUND


def test_onepass_chunked(golden):
    """fwd.chunk_rows forced small on the tiny models: body chunks of 3 + 3 + 1 images, ragged head sub-chunks"""
    g, vae, ar = _tiny_models(golden, 'rqt_tiny.npz', C.RQT_TINY)
    idx = np.arange(7) % g['codes'].shape[0]
    codes, cond = G(g['codes'][idx], torch.long), G(g['cond'][idx], torch.long)
    ar.forward_mode = 'one_pass'
    whole = ar(codes, vae, cond=cond)
    for rows in (3 * 16, 20):
        ar._eng().set_option('fwd.chunk_rows', rows)
        out = ar(codes, vae, cond=cond)
        err = np.abs(N(out) - g['logits'][idx])
        print(f'one-pass rqt_tiny, fwd.chunk_rows = {rows}: logits max err {err.max():.4f} mean {err.mean():.5f}; '
              f'max diff to one chunk {float((out - whole).abs().max()):.5f}')
        assert err.max() < 0.06 and err.mean() < 0.01
        lp = ar.log_probs(codes, vae, cond=cond)
        assert np.abs(N(lp) - _logp64(N(out), N(codes))).max() < LOGP_F64_BOUND
    gt, vaet, art = _tiny_models(golden, 'rqt_tiny_txt.npz', C.RQT_TINY_TXT)
    idx = np.arange(5) % gt['codes'].shape[0]
    codes, cond = G(gt['codes'][idx], torch.long), G(gt['cond'][idx], torch.long)
    art.forward_mode = 'one_pass'
    art._eng().set_option('fwd.chunk_rows', 2 * (C.RQT_TINY_TXT['block_size_cond'] - 1 + 16) + 3)      # 2 + 2 + 1 images
    seq, cl = art(codes, vaet, cond=cond)
    err = np.abs(N(seq) - gt['logits'][idx])
    assert err.max() < 0.06 and err.mean() < 0.01
    art.forward_mode = 'stepped'
    seq_s, cl_s = art(codes, vaet, cond=cond)
    assert float((cl - cl_s).abs().max()) < 0.02 and float((seq - seq_s).abs().max()) < 0.02


def test_onepass_causality_and_determinism(golden):
    g, vae, ar = _tiny_models(golden, 'rqt_tiny.npz', C.RQT_TINY)
    codes, cond = G(g['codes'], torch.long), G(g['cond'], torch.long)
    (B, H, W, D) = codes.shape
    V = C.RQT_TINY['vocab_size']
    ar.forward_mode = 'one_pass'
    run = lambda c, cn=cond: ar(c.reshape(B, H, W, D).contiguous(), vae, cond=cn).reshape(B, H * W, D, -1)
    base = run(codes)
    assert torch.equal(base, run(codes))                             # two calls are bit-identical
    flat = codes.reshape(B, H * W, D)
    for q in range(H * W):
        ch = flat.clone()
        ch[:, q, :] = (ch[:, q, :] + 1 + torch.arange(D, device=DEV)) % V
        out = run(ch)
        assert torch.equal(out[:, :q], base[:, :q]) and torch.equal(out[:, q, 0], base[:, q, 0])
        assert not torch.equal(out[:, q, 1:], base[:, q, 1:])
        for d in range(D):
            ch = flat.clone()
            ch[:, q, d] = (ch[:, q, d] + 7) % V
            out = run(ch)
            assert torch.equal(out[:, :q], base[:, :q]) and torch.equal(out[:, q, :d + 1], base[:, q, :d + 1])
    perm = torch.roll(torch.arange(B, device=DEV), 1)
    assert torch.equal(run(flat[perm], cond[perm].contiguous()), base[perm])      # permuting the images permutes the logits


# ---------------------------------------------------------------------------------------------- 11: the log-softmax kernel alone
def test_log_probs_vs_float64(big, golden):
    """log_probs against float64 log_softmax of the one-pass logits of the same inputs, gathered at the codes (V = 16384, fp32 online
    max / sum): measured maximum 1.58e-6 on the MI355X (log-probabilities of -7.9 .. -11.7, fp32 spacing 9.5e-7), bound 3.16e-6 =
    2 x the measured maximum.  compute_loss(forward(xs), xs) equals -log_probs(xs).mean() within the same bound, and
    compute_codebook_loss / compute_cond_loss equal F.cross_entropy on the same logits."""
    ar, cfg, g, aux, codes, cond = big
    ar.forward_mode = 'one_pass'
    try:
        codes8, cond8 = codes.repeat(4, 1, 1, 1), cond.repeat(4, 1)
        codes8[2:] = (codes8[2:] * 7 + 11) % cfg['vocab_size']       # other codes than the fixture's
        logits = ar(codes8, aux, cond=cond8)
    finally:
        ar.forward_mode = 'stepped'
    lp = ar.log_probs(codes8, aux, cond=cond8)
    assert lp.shape == codes8.shape and lp.dtype == torch.float32
    want = torch.gather(F.log_softmax(logits.double(), -1), -1, codes8.unsqueeze(-1)).squeeze(-1)
    e = float((lp.double() - want).abs().max())
    print(f'log_probs vs float64 log_softmax of the same logits (in1400m, 8 images): max err {e:.3g}, log-probabilities '
          f'{float(lp.min()):.2f} .. {float(lp.max()):.2f}')
    assert e < LOGP_F64_BOUND
    loss = float(ar.compute_loss(logits.double(), codes8))
    assert abs(loss + float(lp.double().mean())) < LOGP_F64_BOUND
    per = ar.compute_codebook_loss(logits, codes8)
    ce = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), codes8.reshape(-1), reduction='none').reshape(-1, 4).mean(0)
    assert torch.equal(per, ce)
    gt, vaet, art = _tiny_models(golden, 'rqt_tiny_txt.npz', C.RQT_TINY_TXT)
    ct, cdt = G(gt['codes'], torch.long), G(gt['cond'], torch.long)
    art.forward_mode = 'one_pass'
    seq, cl = art(ct, vaet, cond=cdt)
    lpt, clp = art.log_probs(ct, vaet, cond=cdt)
    assert torch.equal(art.compute_cond_loss(cl, cdt), F.cross_entropy(cl.reshape(-1, cl.shape[-1]), cdt[:, 1:].reshape(-1)))
    wantc = torch.gather(F.log_softmax(cl.double(), -1), -1, cdt[:, 1:].unsqueeze(-1)).squeeze(-1)
    assert float((clp.double() - wantc).abs().max()) < LOGP_F64_BOUND
    assert abs(float(art.compute_cond_loss(cl.double(), cdt)) + float(clp.double().mean())) < LOGP_F64_BOUND


# ---------------------------------------------------------------------------------------------- 12: sampling is untouched
def test_sampling_untouched_by_onepass(big, golden):
    """sample() with a fixed seed and captured graphs gives the same codes before and after a one-pass call at a larger batch on
    the same module (its workspace is its own; the graphs' addresses stay valid), and the default forward() is still eng.logits."""
    ar, cfg, g, aux, codes, cond = big
    gt, vae, tiny = _tiny_models(golden, 'rqt_tiny.npz', C.RQT_TINY)
    for m, a, cs, cn, k in ((tiny, vae, G(gt['codes'], torch.long), G(gt['cond'], torch.long), 50), (ar, aux, codes, cond, 1024)):
        assert m.forward_mode == 'stepped'
        m.use_graph = True
        part = torch.zeros_like(cs)
        torch.cuda.manual_seed_all(123)
        before = m.sample(part, a, cond=cn, top_k=k, top_p=0.95)
        reps = 16
        lp = m.log_probs(cs.repeat(reps, 1, 1, 1), a, cond=cn.repeat(reps, 1))
        m.forward_mode = 'one_pass'
        big_out = m(cs.repeat(reps, 1, 1, 1), a, cond=cn.repeat(reps, 1))
        m.forward_mode = 'stepped'
        assert torch.isfinite(lp).all() and torch.isfinite(big_out).all()
        torch.cuda.manual_seed_all(123)
        after = m.sample(part, a, cond=cn, top_k=k, top_p=0.95)
        assert torch.equal(before, after)
        stepped = m(cs, a, cond=cn)
        eng_logits = m._eng().logits(cs, cn, m._checked_codebooks(a))
        assert torch.equal(stepped, eng_logits)                        # the default forward(): bit for bit the stepped engine
        assert torch.equal(big_out[:cs.shape[0]], big_out[cs.shape[0]:2 * cs.shape[0]])
        print(f'max |one-pass - stepped| logits: {float((big_out[:cs.shape[0]] - stepped).abs().max()):.4f}')
        del big_out, lp


# ---------------------------------------------------------------------------------------------- 13: speed
def _time_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def test_onepass_is_three_times_faster_at_8_images(big):
    """1.4B model, 8 images, device events after warm-up: the one-pass forward takes at most one third of the stepped forward's time.
    (The stepped pass streams the weight set 64 times and the head stack 256 times; the one-pass needs ~2 TFLOP.  Expected ratio
    above 10; 3 leaves room for a shared machine.)"""
    ar, cfg, g, aux, codes, cond = big
    codes8, cond8 = codes.repeat(4, 1, 1, 1), cond.repeat(4, 1)
    res = {}
    for mode in ('stepped', 'one_pass', 'stepped', 'one_pass'):
        ar.forward_mode = mode
        try:
            ar(codes8, aux, cond=cond8)                               # warm-up of this shape
            res.setdefault(mode, []).append(_time_ms(lambda: ar(codes8, aux, cond=cond8), 3))
        finally:
            ar.forward_mode = 'stepped'
    stepped, one = min(res['stepped']), min(res['one_pass'])
    lp = _time_ms(lambda: ar.log_probs(codes8, aux, cond=cond8), 3)
    print(f'in1400m, 8 images: stepped forward {stepped:.1f} ms, one-pass forward {one:.1f} ms ({stepped / one:.1f}x), log_probs {lp:.1f} ms')
    assert one * 3 <= stepped
