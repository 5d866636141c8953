"""Classifier-free guidance on the MI355X (`pytest -m gpu`): RQTransformer.sample_guided over rqamd_rqt_sample_guided, and
rqamd_guide_logits.  A guided call runs the engine over 2B rows (images under `cond`, then their twins under `uncond`); the sampler
draws row b from guide(c_b, u_b, s) with the filter and Philox counter of row b and writes the code to both twins.  Apart from
guide_logits against fp64 and the statistical test every comparison is exact.  Captured graphs are on unless a test says otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import configs as C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import guided_sampling_cases as G  # noqa: E402
import masked_sampling_cases as M  # noqa: E402
from sample_stats import sample_stats_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()                      # raises if librqamd.so is missing: no fallback
    return _native


def _setup(cfg, B, seed=41):
    ar, aux = M.model(cfg, seed, DEV)
    cond = M.cond_for(cfg, B, DEV)
    uncond = G.uncond_for(cfg, cond)
    assert bool((cond != uncond).any(dim=1).all())
    H, W, D = cfg['block_size']
    return ar, aux, cond, uncond, torch.zeros((B, H, W, D), dtype=torch.long, device=DEV)


@pytest.fixture(scope='module')
def tiny3(nat):
    """RQT_TINY (4x4x4, V 500) with seeded weights, 3 images"""
    return _setup(C.RQT_TINY, 3)


# ---------------------------------------------------------------------------------------------- 1. s = 1 identity
IDENTITY = {'b2': (C.RQT_TINY, 2, {}), 'b40_80_rows': (C.RQT_TINY, 40, {}), 'text_prefix_b3': (C.RQT_TINY_TXT, 3, {}),
            'bf16_and_fp16_engine': (C.RQT_TINY, 2, dict(amp=True))}


@pytest.mark.parametrize('config', sorted(IDENTITY))
def test_guided_s1_identity(nat, config):
    cfg, B, extra = IDENTITY[config]
    ar, aux, cond, uncond, zeros = _setup(cfg, B)
    for kw in G.SAMPLERS:
        G.check_s1_identity(ar, aux, zeros, cond, uncond, seed=5, **kw, **extra)
    if extra:                                              # the fp16 engine above; the bf16 engine of the same model
        G.check_s1_identity(ar, aux, zeros, cond, uncond, seed=5, **G.SAMPLERS[1])


# ---------------------------------------------------------------------------------------------- 2. graph == eager == uncached
def test_guided_graph_eager_uncached_agree(tiny3):
    ar, aux, cond, uncond, zeros = tiny3
    kw = dict(cond=cond, uncond=uncond, guidance_scale=3.0, top_k=50, top_p=0.9)
    M.seed_all(7)
    a = ar.sample_guided(zeros, aux, **kw)
    ar.use_graph = False
    try:
        M.seed_all(7)
        b = ar.sample_guided(zeros, aux, **kw)
    finally:
        ar.use_graph = True
    M.seed_all(7)
    c = ar.sample_guided(zeros, aux, cached=False, **kw)
    assert torch.equal(a, b), 'captured graphs and eager launches differ'
    assert torch.equal(a, c), 'cached=True and cached=False differ'


# ---------------------------------------------------------------------------------------------- 3. greedy == argmax / support
def test_guided_greedy_is_argmax_tiny(nat):
    ar, aux, cond, uncond, zeros = _setup(C.RQT_TINY, 4)
    M.seed_all(3)
    xs = ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=2.5, top_k=1)
    G.check_guided_support(nat, ar, aux, xs, cond, uncond, 2.5, 1)


@pytest.fixture(scope='module')
def wide4(nat):
    """RQT_WIDE (E 1536, V 16384, 8x8x4), 4 images: the sampler rows at the product's width"""
    return _setup(C.RQT_WIDE, 4, seed=43)


def test_guided_greedy_is_argmax_real_width(nat, wide4):
    ar, aux, cond, uncond, zeros = wide4
    M.seed_all(3)
    xs = ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=2.5, top_k=1)
    G.check_guided_support(nat, ar, aux, xs, cond, uncond, 2.5, 1)


def test_guided_support_real_width(nat, wide4):
    ar, aux, cond, uncond, zeros = wide4
    M.seed_all(4)
    xs = ar.sample_guided(zeros, aux, cond=cond, uncond=uncond, guidance_scale=2.5, top_k=1024, top_p=0.95)
    G.check_guided_support(nat, ar, aux, xs, cond, uncond, 2.5, 1024)


# ---------------------------------------------------------------------------------------------- 4. graph keys
def test_guided_graph_keys(nat):
    """plain, guided (s = 3), masked plain, guided (s = 1.5), guided (s = 3), plain on one model: no call replays a graph captured
    for another form or another scale"""
    ar, aux, cond, uncond, zeros = _setup(C.RQT_TINY, 3)
    kw = dict(top_k=50, top_p=0.9)
    gk = dict(cond=cond, uncond=uncond, **kw)
    keep_t = torch.from_numpy(M.replay_mask(3, 4, 4, 4, seed=25)).to(DEV)
    M.seed_all(1)
    p1 = ar.sample(zeros, aux, cond=cond, **kw)
    M.seed_all(2)
    g3a = ar.sample_guided(zeros, aux, guidance_scale=3.0, **gk)
    ar.sample(G.random_codes((3, 4, 4, 4), 500, 3, DEV), aux, cond=cond, keep_mask=keep_t, **kw)
    M.seed_all(2)
    g15 = ar.sample_guided(zeros, aux, guidance_scale=1.5, **gk)
    M.seed_all(2)
    g3b = ar.sample_guided(zeros, aux, guidance_scale=3.0, **gk)
    M.seed_all(1)
    p2 = ar.sample(zeros, aux, cond=cond, **kw)
    assert torch.equal(p1, p2), 'the plain call changed after guided and masked calls on the same handle'
    assert torch.equal(g3a, g3b), 'guided (s = 3) changed after a guided call with another scale'
    assert not torch.equal(g3a, g15), 'guided calls with s = 3 and s = 1.5 returned the same codes'
    fresh, aux2 = M.model(C.RQT_TINY, 41, DEV)             # and all of them are what a handle that saw nothing else returns
    M.seed_all(2)
    assert torch.equal(fresh.sample_guided(zeros, aux2, guidance_scale=1.5, **gk), g15)


# ---------------------------------------------------------------------------------------------- 5. guided + masked replay
@pytest.mark.parametrize('start_loc', [(0, 0), (1, 2)])
def test_guided_masked_replay(tiny3, start_loc):
    ar, aux, cond, uncond, _ = tiny3
    partial = G.random_codes((3, 4, 4, 4), 500, 6, DEV)    # (the prefix before start_loc is given)
    codes0 = G.check_guided_replay(ar, aux, partial, cond, uncond, 3.0, seed=13, mask_seed=21, start_loc=start_loc, top_k=50, top_p=0.9)
    start = start_loc[0] * 4 + start_loc[1]
    assert torch.equal(codes0.view(3, 16, 4)[:, :start], partial.view(3, 16, 4)[:, :start])
    assert not torch.equal(codes0, partial)


# ---------------------------------------------------------------------------------------------- 6. guide_logits against fp64
@pytest.mark.parametrize('shape', [(5, 16384), (3, 499)])
def test_guide_logits_fp64(nat, shape):
    G.check_guide_logits(nat, shape[0], shape[1], DEV, seed=shape[1])


# ---------------------------------------------------------------------------------------------- 7. statistics
def test_guided_draws_follow_the_guided_conditionals(nat, golden):
    """The martingale test of tests/test_gpu_sample_stats.py on guided draws: 4096 images (262 144 draws), T 0.9 / top-k 50 / top-p 0.9,
    s = 3, cond = i % 10, uncond = (cond + 5) % 10.  q = filtered_probs(guide_logits(Lc, Lu, 3)) with Lc | Lu the two halves of ONE
    teacher-forced pass over cat(xs, xs): sum [log q(x) + H(q)] is a zero-mean martingale, |z| < 5, and at most draws // 20000 draws
    outside the filtered support.  Power: against the cond-only conditionals filtered_probs(Lc) more than draws // 100 of the same
    draws fall outside the support, or |z| > 10.  (The numpy oracle sampling exactly from the guided conditionals, 256 images: z =
    -0.97 with 0 outside; against cond-only 6.1 % outside, z = +6.8.)"""
    g = golden('rqt_tiny_sample_stats.npz')
    cfg = C.RQT_TINY
    from rqvae.models.rqvae import RQVAE
    from rqvae.models.rqtransformer import RQTransformer
    hps, dd = C.VAE_TINY                                   # the models of tests/test_gpu_sample_stats.py, from the fixture's seeds
    aux = RQVAE(**hps, ddconfig=dd, checkpointing=False)
    aux.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqvae_param_shapes(hps, dd), int(g['vae_seed'])).items()})
    ar = RQTransformer(cfg)
    ar.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqt_param_shapes(cfg), int(g['seed'])).items()})
    aux, ar = aux.to(DEV).eval(), ar.to(DEV).eval()
    n, T, K, P, S = 4096, 0.9, 50, 0.9, 3.0
    part, cond, _ = sample_stats_inputs(cfg, 'cond', n)
    cond_t = torch.from_numpy(cond).to(DEV)
    uncond_t = (cond_t + 5) % 10
    M.seed_all(99)
    xs = ar.sample_guided(torch.from_numpy(part).to(DEV), aux, cond=cond_t, uncond=uncond_t, guidance_scale=S, temperature=T, top_k=K, top_p=P)
    L = ar.teacher_forced_logits(torch.cat([xs, xs]), aux, cond=torch.cat([cond_t, uncond_t]))            # (2n, H, W, D, V)
    V = L.shape[-1]
    Lc, Lu = L[:n].reshape(-1, V), L[n:].reshape(-1, V)
    rows_g = nat.guide_logits(Lc, Lu, S).cpu().numpy()
    rows_c = Lc.cpu().numpy()
    draws = xs.reshape(-1).cpu().numpy()

    def z_of(q):
        qx = q[np.arange(q.shape[0]), draws]
        inside = qx > 0
        with np.errstate(divide='ignore', invalid='ignore'):
            lq = np.where(q > 0, np.log(q), 0.0)
        ent = -(q * lq).sum(-1)
        var = (q * lq * lq).sum(-1) - ent ** 2
        s = (np.log(qx[inside]) + ent[inside]).sum()
        return float(s / np.sqrt(var[inside].sum())), int((~inside).sum())

    def probs(rows):
        return np.concatenate([oracle.sampler.filtered_probs(rows[i:i + 16384], temperature=T, top_k=K, top_p=P) for i in range(0, rows.shape[0], 16384)])
    z, outside = z_of(probs(rows_g))
    z_c, outside_c = z_of(probs(rows_c))
    print(f'guided sampling self-consistency (s {S}, T {T}, top-k {K}, top-p {P}; {draws.size} draws): z = {z:+.2f} (bound 5), {outside} draws '
          f'outside the filtered support; against the cond-only conditionals z = {z_c:+.1f}, {outside_c} outside')
    assert outside <= draws.size // 20000, f'{outside} draws outside the filtered support of their guided conditional'
    assert abs(z) < 5.0
    assert outside_c > draws.size // 100 or abs(z_c) > 10.0
