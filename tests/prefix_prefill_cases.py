"""Shared by tests/test_emu_prefix_prefill.py (host emulator) and tests/test_gpu_prefix_prefill.py (MI355X): the checks of the one-pass
prefix prefill -- the engine option "prefix.one_pass", rqamd_rqt_step_prefill and RQTransformer.prefix_mode = 'one_pass'.

Two kinds of comparison:
  bounded    logits of the positions after a prefilled prefix against the reference's own (the fixtures under tests/golden/) with the
             bound the existing tests of the same model and cache format use, and against the engine's stepped logits of the same inputs
             with the project's path-to-path bound (0.02 per logit: ONEPASS_LOGP / 2 of tests/sample_logp_cases.py; same arithmetic,
             other GEMM tiles).  The stepped side is the engine's stepped teacher-forced pass over the same codes: a body-only step and
             a step whose head runs launch the same body kernels, so these ARE the logits behind a stepped prefix, whatever n0 is --
             computed once per model and shared.
  exact      inside the mode every sampling form draws the same codes; with the option off nothing changes."""
import os
import sys

import numpy as np
import torch

import oracle
from oracle import configs as C

import masked_sampling_cases as M
from sample_logp_cases import ONEPASS_LOGP

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import long_cases as L  # noqa: E402

PATH_LOGIT = ONEPASS_LOGP / 2            # 0.02 per logit, one-pass against stepped
REF_TINY = (0.06, 0.01)                  # the fixture tests' own bound on the tiny models (max, mean), emulator and GPU
# rqt_long_*: the bounds of tests/test_emu_long_context.py / tests/test_gpu_long_context.py (B_LOGITS there: twice the measured error)
REF_LONG = {'emu': (min(0.06, 2 * 0.0104), min(0.01, 2 * 0.00177)), 'gpu': (min(0.06, 2 * 0.0100), min(0.01, 2 * 0.00173))}
# tiny model with RQAMD_KV=int8k / int8kv: tests/test_emu_kernels.py::test_emu_rqt_int8k_key_cache / tests/test_gpu_parity.py::test_rqt_int8k_key_cache_tiny
REF_INT8 = {'emu': (0.06, 0.01), 'gpu': (0.03, 0.005)}
REF_F16 = (0.004, 0.0006)                # amp=True on the tiny fixture: tests/test_gpu_parity.py (F16_MAX_ERR, F16_MEAN_ERR)

TINY_N0 = (1, 2, 7, 8, 9, 15)
TXT_N0 = (1, 5, 15)
VARIANTS = {'tuple': 'RQT_TINY_TUPLE', 'heads': 'RQT_TINY_HEADS', 'nocumsum': 'RQT_TINY_NOCUMSUM'}
SAMPLER = dict(top_k=50, top_p=0.9)


def T(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------ models of the fixtures
def _load(cfg, seed, device):
    from rqvae.models.rqtransformer import RQTransformer
    ar = RQTransformer(cfg)
    ar.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqt_param_shapes(cfg), seed, cfg).items()}, strict=True)
    return ar.to(device).eval()


_CASES = {}


def case(golden, name, device, amp=False):
    """One fixture, its model and the engine's stepped logits of the fixture's inputs -- built once per (fixture, device, RQAMD_KV, amp),
    shared and never written to.  name: 'tiny', 'txt', a key of VARIANTS, 'txt300' or 'map'"""
    key = (name, str(device), os.environ.get('RQAMD_KV', ''), bool(amp))
    if key in _CASES:
        return _CASES[key]
    if name in ('txt300', 'map'):
        cfg = L.txt_cfg(300, n_body=2) if name == 'txt300' else L.map_cfg()
        g = golden(f'rqt_long_{name}.npz')
        cb, codes, cond = L.inputs(cfg, int(g['input_seed']))
        H, W, D = cfg['block_size']
        pos = np.arange(H * W) if name == 'txt300' else np.asarray(g['pos'])
        ref = g['logits'].reshape(2, len(pos), D, -1)
        aux = M.Aux(cb, D, device)
    else:
        fname, cfg = {'tiny': ('rqt_tiny.npz', C.RQT_TINY), 'txt': ('rqt_tiny_txt.npz', C.RQT_TINY_TXT)}.get(
            name, (f'rqt_var_{name}.npz', getattr(C, VARIANTS.get(name, 'RQT_TINY'))))
        g = golden(fname)
        hps, dd = C.VAE_TINY
        cb = oracle.make_params(oracle.rqvae_param_shapes(hps, dd), int(g['vae_seed']))['quantizer.codebooks.0.weight'][:-1]
        codes, cond = g['codes'].astype(np.int64), g['cond'].astype(np.int64)
        H, W, D = cfg['block_size']
        pos = np.arange(H * W)
        ref = g['logits'].reshape(codes.shape[0], H * W, D, -1)
        aux = None if name == 'tuple' else M.Aux(cb, D, device)
    ar = _load(cfg, int(g['seed']), device)
    c = dict(cfg=cfg, ar=ar, aux=aux, codes=T(codes, device, torch.long), cond=T(cond, device, torch.long), pos=pos, ref=ref, amp=bool(amp),
             vocab=list(ar.vocab_size))
    B = codes.shape[0]
    c['stepped'] = ar.teacher_forced_logits(c['codes'], aux, cond=c['cond'], amp=amp).cpu().numpy().reshape(B, H * W, D, -1)[:, pos]
    _CASES[key] = c
    return c


def forget_cases():
    _CASES.clear()


# ------------------------------------------------------------------------------------------------ 1.-3. logits after the prefill
def prefill_logits(c, n0, idx=None, chunk_rows=None):
    """step_begin with the fixture's codes and cond (images idx, or all), step_prefill(n0), then step_logits(pos, 0 .. D-1) for every
    pos >= n0 in order -> {stored index i: (B, D, V) logits of position c['pos'][i]}"""
    ar = c['ar']
    eng = ar._eng(c['amp'])
    H, W, D = ar.block_size
    codes, cond = c['codes'], c['cond']
    if idx is not None:
        sel = torch.as_tensor(idx, device=codes.device)
        codes, cond = codes[sel].contiguous(), cond[sel].contiguous()
    cbs = ar._checked_codebooks(c['aux'])
    if chunk_rows is not None:
        eng.set_option('fwd.chunk_rows', chunk_rows)
    try:
        # the cache holds the keys and values of OTHER codes under another conditioning first (body-only steps over the whole map): a
        # prefill that left any cache row alone would be seen -- case() has just stepped the very inputs of this call on this engine
        vmax = torch.tensor(c['vocab'], dtype=torch.long, device=codes.device)
        vc = max(int(c['cfg']['vocab_size_cond']), 1)
        eng.step_begin((codes + 7) % vmax, ((cond + 1) % vc).reshape(codes.shape[0], -1), cbs)
        for pos in range(H * W):
            eng.step_logits(pos, -1)
        eng.step_end()
        eng.step_begin(codes, cond.reshape(codes.shape[0], -1), cbs)
        eng.step_prefill(n0)
        where = {int(p): i for i, p in enumerate(c['pos'])}
        out = {}
        for pos in range(n0, H * W):
            rows = []
            for d in range(D):
                lg = eng.step_logits(pos, d)
                if pos in where:
                    rows.append(lg.cpu().numpy().copy())
            if pos in where:
                out[where[pos]] = np.stack(rows, 1)
        eng.step_end()
    finally:
        if chunk_rows is not None:
            eng.set_option('fwd.chunk_rows', 4096)
    return out


def check_prefill_logits(c, n0, ref_bound, what, idx=None, chunk_rows=None):
    """the logits of every stored position >= n0 behind a prefix of n0 positions filled in one pass: against the reference within
    ref_bound (max, mean) and against the stepped path within PATH_LOGIT.  Columns beyond a depth's vocabulary are compared nowhere: the
    stepping API masks them (LogitMask), the fixtures do not."""
    got = prefill_logits(c, n0, idx, chunk_rows)
    assert got, (what, n0)
    rows = slice(None) if idx is None else np.asarray(idx)
    e_ref, e_path = [], []
    for i, lg in sorted(got.items()):
        for d, v in enumerate(c['vocab']):
            e_ref.append(np.abs(lg[:, d, :v].astype(np.float64) - c['ref'][rows, i, d, :v]).ravel())
            e_path.append(np.abs(lg[:, d, :v] - c['stepped'][rows, i, d, :v]).ravel())
    e_ref, e_path = np.concatenate(e_ref), np.concatenate(e_path)
    print('prefix prefill %s, n0 = %d: %d positions, vs the reference max %.4f mean %.5f, vs the stepped prefix max %.5f'
          % (what, n0, len(got), e_ref.max(), e_ref.mean(), e_path.max()))
    assert e_ref.max() < ref_bound[0] and e_ref.mean() < ref_bound[1], (what, n0)
    assert e_path.max() < PATH_LOGIT, (what, n0)
    return e_ref.max(), e_ref.mean(), e_path.max()


def check_chunked(c, ref_bound):
    """tiny model (9 tokens per image at n0 = 9), 5 images, fwd.chunk_rows = 20: chunks of 2 + 2 + 1 images"""
    n = c['codes'].shape[0]
    return check_prefill_logits(c, 9, ref_bound, 'chunks of 2 + 2 + 1 images', idx=np.arange(5) % n, chunk_rows=20)


# ------------------------------------------------------------------------------------------------ 4.-7., 9. the sampling forms
def sampling_setup(device, B=3, seed=41):
    """tiny model, B images, a conditioning and a map of valid codes (the prefix of a completion call)"""
    cfg = C.RQT_TINY
    ar, aux = M.model(cfg, seed, device)
    cond = M.cond_for(cfg, B, device)
    H, W, D = cfg['block_size']
    partial = T(np.random.default_rng(seed + 1).integers(0, cfg['vocab_size'], (B, H, W, D)), device, torch.long)
    return ar, aux, cond, partial


def prefix_mask(H, W, n0, device):
    m = torch.zeros(H * W, dtype=torch.bool, device=device)
    m[:n0] = True
    return m.view(H, W)


def check_forms_agree(device, start=(2, 1), seed=11):
    """inside prefix_mode = 'one_pass': start_loc == the same leading prefix as keep_mask == per-image tensors == return_log_probs() ==
    use_graph=False, bit for bit; codes at positions >= n0 of partial_sample change nothing; sample_guided(guidance_scale=1) == the first
    half of sample over the 2B rows"""
    ar, aux, cond, partial = sampling_setup(device)
    ar.prefix_mode = 'one_pass'
    B, H, W, D = partial.shape
    n0 = start[0] * W + start[1]

    def run(fn):
        M.seed_all(seed)
        return fn()
    base = run(lambda: ar.sample(partial, aux, cond=cond, start_loc=start, **SAMPLER))
    flat, bflat = partial.view(B, H * W, D), base.view(B, H * W, D)
    assert torch.equal(bflat[:, :n0], flat[:, :n0]), 'the prefix was changed'
    assert int(base.min()) >= 0 and int(base.max()) < 500
    assert not torch.equal(bflat[:, n0:], flat[:, n0:]), 'nothing was drawn'
    masked = run(lambda: ar.sample(partial, aux, cond=cond, keep_mask=prefix_mask(H, W, n0, device), **SAMPLER))
    assert torch.equal(masked, base), 'keep_mask prefix != start_loc'
    per = run(lambda: ar.sample(partial, aux, cond=cond, start_loc=start, temperature=torch.ones(B, device=device),
                                top_k=torch.full((B,), SAMPLER['top_k'], dtype=torch.long, device=device),
                                top_p=torch.full((B,), SAMPLER['top_p'], dtype=torch.float32, device=device)))
    assert torch.equal(per, base), 'per-image call != scalar call'
    with ar.return_log_probs():
        lp_codes, lp = run(lambda: ar.sample(partial, aux, cond=cond, start_loc=start, **SAMPLER))
    assert torch.equal(lp_codes, base), 'return_log_probs() changed the codes'
    ar.use_graph = False
    try:
        eager = run(lambda: ar.sample(partial, aux, cond=cond, start_loc=start, **SAMPLER))
    finally:
        ar.use_graph = True
    assert torch.equal(eager, base), 'use_graph=False != graphs'
    other = partial.clone()
    other.view(B, H * W, D)[:, n0:] = (other.view(B, H * W, D)[:, n0:] + 7) % 500            # other valid codes after the prefix
    assert torch.equal(run(lambda: ar.sample(other, aux, cond=cond, start_loc=start, **SAMPLER)), base), 'codes after the prefix were read'
    # guided at scale 1 == the first half of the unguided call over the 2B rows
    uncond = M.cond_for(C.RQT_TINY, B, device, seed=6)
    guided = run(lambda: ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=1.0, start_loc=start, **SAMPLER))
    twice = run(lambda: ar.sample(torch.cat([partial, partial]), aux, cond=torch.cat([cond, uncond]), start_loc=start, **SAMPLER))
    assert torch.equal(guided, twice[:B]), 'sample_guided(1.0) != first half of sample over 2B rows'
    # the torch sampler steps: its prefix goes through step_prefill and leaves the prefix alone too
    ar.sampler = 'torch'
    try:
        tm = run(lambda: ar.sample(partial, aux, cond=cond, start_loc=start, **SAMPLER))
    finally:
        ar.sampler = 'philox'
    assert torch.equal(tm.view(B, H * W, D)[:, :n0], flat[:, :n0]) and int(tm.min()) >= 0 and int(tm.max()) < 500
    return ar, aux, cond, partial, base, lp


def check_stale_cache(device, start=(2, 1), seed=12):
    """a full sample() on the handle first, then the prefix call == the same prefix call on a fresh engine"""
    ar, aux, cond, partial = sampling_setup(device)
    ar.prefix_mode = 'one_pass'
    M.seed_all(3)
    ar.sample(torch.zeros_like(partial), aux, cond=cond, **SAMPLER)
    M.seed_all(seed)
    after = ar.sample(partial, aux, cond=cond, start_loc=start, **SAMPLER)
    fresh, aux2, _, _ = sampling_setup(device)
    fresh.prefix_mode = 'one_pass'
    M.seed_all(seed)
    assert torch.equal(fresh.sample(partial, aux2, cond=cond, start_loc=start, **SAMPLER), after)


def check_conditioned_on_prefix(ar, aux, cond, partial, codes, lp, start=(2, 1)):
    """lp.model of the draws (from check_forms_agree) against log_probs(codes) within ONEPASS_LOGP at the drawn positions -- the draws saw
    the prefix --, NaN at the prefix positions; lp.draw +0.0 there"""
    B, H, W, D = codes.shape
    n0 = start[0] * W + start[1]
    model, draw = lp.model.view(B, H * W, D).cpu(), lp.draw.view(B, H * W, D).cpu()
    assert lp.model_uncond is None
    assert bool(torch.isnan(model[:, :n0]).all()), 'model log-probabilities at prefix positions'
    assert bool((draw[:, :n0] == 0).all()) and not bool(torch.signbit(draw[:, :n0]).any()), 'draw log-probabilities at prefix positions'
    full = ar.log_probs(codes, aux, cond=cond).view(B, H * W, D).cpu()
    err = float((model[:, n0:] - full[:, n0:]).abs().max())
    print('prefix prefill, model log-probabilities of the draws vs log_probs(codes): max %.5f' % err)
    assert err < ONEPASS_LOGP
    assert bool((draw[:, n0:] <= 0).all()) and bool(torch.isfinite(draw[:, n0:]).all())
    # (the comparison has teeth: under another prefix the same codes have other log-probabilities)
    other = codes.clone()
    other.view(B, H * W, D)[:, :n0] = (other.view(B, H * W, D)[:, :n0] + 7) % 500
    shifted = ar.log_probs(other, aux, cond=cond).view(B, H * W, D).cpu()
    assert float((model[:, n0:] - shifted[:, n0:]).abs().max()) > ONEPASS_LOGP


def check_graphs(device, start=(2, 1)):
    """stepped and one-pass calls alternated with log_probs between them: after the first call of each kind nothing is captured again"""
    ar, aux, cond, partial = sampling_setup(device)

    def call(mode):
        ar.prefix_mode = mode
        M.seed_all(5)
        return ar.sample(partial, aux, cond=cond, start_loc=start, **SAMPLER)
    first = {m: call(m) for m in ('stepped', 'one_pass')}
    ar.log_probs(first['stepped'], aux, cond=cond)
    n = ar._eng().graph_captures()
    assert n >= 1
    for m in ('stepped', 'one_pass', 'one_pass', 'stepped'):
        assert torch.equal(call(m), first[m]), m
        ar.log_probs(first[m], aux, cond=cond)
        assert ar._eng().graph_captures() == n, m
    return first


def check_default_untouched(device, start=(2, 1)):
    """"prefix.one_pass" = 0 (set, or set to 1 and back) == a handle on which the option was never set; the default mode is 'stepped'"""
    from rqvae.models.rqtransformer import RQTransformer
    assert RQTransformer(C.RQT_TINY).prefix_mode == 'stepped'
    ar, aux, cond, partial = sampling_setup(device)
    M.seed_all(5)
    never = ar.sample(partial, aux, cond=cond, start_loc=start, **SAMPLER)
    assert not hasattr(ar._eng(), '_prefix_one_pass')                     # the default never touches the option
    ar2, aux2, _, _ = sampling_setup(device)
    ar2._eng().set_option('prefix.one_pass', 0)
    M.seed_all(5)
    assert torch.equal(ar2.sample(partial, aux2, cond=cond, start_loc=start, **SAMPLER), never)
    ar2._eng().set_option('prefix.one_pass', 1)
    ar2._eng().set_option('prefix.one_pass', 0)
    M.seed_all(5)
    assert torch.equal(ar2.sample(partial, aux2, cond=cond, start_loc=start, **SAMPLER), never)


# ------------------------------------------------------------------------------------------------ 8. errors
def check_errors(nat, device):
    """every refusal happens on the host, before anything is launched"""
    import pytest
    ar, aux, cond, partial = sampling_setup(device, B=2)
    eng = ar._eng()
    cbs = ar._checked_codebooks(aux)
    HW = 16
    with pytest.raises(nat.RqamdError, match='step_begin'):
        eng.step_prefill(3)                                                # before step_begin
    eng.step_begin(partial, cond, cbs)
    for bad in (0, HW, -1, HW + 5):
        with pytest.raises(ValueError, match='n_pos'):
            eng.step_prefill(bad)
    eng.step_prefill(3)
    with pytest.raises(nat.RqamdError, match='step_begin'):
        eng.step_prefill(3)                                                # twice
    eng.step_logits(3, 0)
    eng.step_end()
    eng.step_begin(partial, cond, cbs)
    eng.step_logits(0, -1)
    with pytest.raises(nat.RqamdError, match='step_begin'):
        eng.step_prefill(3)                                                # after a step_logits
    eng.step_end()
    eng.step_begin(partial, cond, cbs)
    eng.step_logits(0, 0)
    with pytest.raises(nat.RqamdError, match='step_begin'):
        eng.step_prefill(3)                                                # after a head step of position 0
    eng.step_end()
    with pytest.raises(nat.RqamdError, match='step_begin'):
        eng.step_prefill(3)                                                # after step_end
    for bad in (2, -1):
        with pytest.raises(ValueError, match='prefix.one_pass'):
            eng.set_option('prefix.one_pass', bad)
    ar.prefix_mode = 'x'
    with pytest.raises(ValueError, match='prefix_mode'):
        ar.sample(partial, aux, cond=cond, start_loc=(1, 0))
    with pytest.raises(ValueError, match='prefix_mode'):
        ar.sample_guided(partial, aux, cond=cond, start_loc=(1, 0))
    ar.init_cache()
    with pytest.raises(ValueError, match='prefix_mode'):
        ar.cached_forward(partial[:, :2], aux, cond=cond, sample_loc=(1, 1, 0))
    ar.prefix_mode = 'stepped'


def check_cached_forward_restart(device):
    """a restarted cached_forward in the mode: the logits of the step, and of the steps that continue it, within PATH_LOGIT of the stepped
    restart's"""
    ar, aux, cond, partial = sampling_setup(device, B=2)
    out = {}
    for mode in ('stepped', 'one_pass'):
        ar.prefix_mode = mode
        ar.init_cache()
        out[mode] = [ar.cached_forward(partial[:, :3], aux, cond=cond, sample_loc=(2, 1, d)).cpu() for d in range(2)]
        out[mode].append(ar.cached_forward(partial[:, :3], aux, cond=cond, sample_loc=(2, 1, 2)).cpu())
    ar.init_cache()
    d = max(float((a - b).abs().max()) for a, b in zip(out['stepped'], out['one_pass']))
    print('prefix prefill, restarted cached_forward: one-pass vs stepped restart %.5f' % d)
    assert d < PATH_LOGIT
