"""Shared by tests/test_emu_kept_runs.py (host emulator) and tests/test_gpu_kept_runs.py (MI355X): the checks of the one-pass fill of
interior kept runs -- the engine option "masked.run_prefill", rqamd_rqt_step_run and RQTransformer.kept_run_mode = 'one_pass'.

The comparisons are those of tests/prefix_prefill_cases.py, whose fixtures, loaders and bounds are used:
  bounded    logits of the positions behind a run that was filled in one pass against the reference's own (tests/golden/) within the
             fixture's bound, and against the engine's stepped logits of the same inputs within PATH_LOGIT (0.02: same arithmetic, other
             GEMM tiles).
  exact      inside the mode every sampling form draws the same codes; with the option off nothing changes; what the pass does not
             serve draws what it draws with the option off."""
import numpy as np
import torch

from oracle import configs as C

import masked_sampling_cases as M
import prefix_prefill_cases as PC
from sample_logp_cases import ONEPASS_LOGP

SAMPLER = PC.SAMPLER
T = PC.T


# ------------------------------------------------------------------------------------------------ 1. logits behind a run
def run_logits(c, runs, heads, idx=None, chunk_rows=None, stale=True):
    """step_begin with the fixture's codes and cond (images idx, or all); positions in order: a run (p0, p1) of `runs` through
    step_run, a position of `heads` through step_logits(pos, 0 .. D-1), every other position body-only
    -> {stored index i: (B, D, V) logits of position c['pos'][i]}"""
    ar = c['ar']
    eng = ar._eng(c['amp'])
    H, W, D = ar.block_size
    HW = H * W
    codes, cond = c['codes'], c['cond']
    if idx is not None:
        sel = torch.as_tensor(idx, device=codes.device)
        codes, cond = codes[sel].contiguous(), cond[sel].contiguous()
    cbs = ar._checked_codebooks(c['aux'])
    starts = dict(runs)
    assert all(1 <= p0 < p1 <= HW - 1 for p0, p1 in runs) and not any(p0 <= p < p1 for p in heads for p0, p1 in runs)
    if chunk_rows is not None:
        eng.set_option('fwd.chunk_rows', chunk_rows)
    try:
        if stale:
            # the cache holds the keys and values of OTHER codes under another conditioning first: a pass that left a row of its run
            # alone, or wrote it elsewhere, is seen in the logits behind it
            vmax = torch.tensor(c['vocab'], dtype=torch.long, device=codes.device)
            vc = max(int(c['cfg']['vocab_size_cond']), 1)
            eng.step_begin((codes + 7) % vmax, ((cond + 1) % vc).reshape(codes.shape[0], -1), cbs)
            for pos in range(HW):
                eng.step_logits(pos, -1)
            eng.step_end()
        eng.step_begin(codes, cond.reshape(codes.shape[0], -1), cbs)
        where = {int(p): i for i, p in enumerate(c['pos'])}
        out, pos = {}, 0
        while pos < HW:
            if pos in starts:
                eng.step_run(pos, starts[pos])
                pos = starts[pos]
                continue
            if pos in heads:
                rows = [eng.step_logits(pos, d).cpu().numpy().copy() for d in range(D)]
                if pos in where:
                    out[where[pos]] = np.stack(rows, 1)
            else:
                eng.step_logits(pos, -1)
            pos += 1
        eng.step_end()
    finally:
        if chunk_rows is not None:
            eng.set_option('fwd.chunk_rows', 4096)
    return out


def heads_behind(runs, HW):
    """p1 and p1 + 1 of every run and the last position (those that lie in no run)"""
    want = {HW - 1}
    for _, p1 in runs:
        want.update((p1, p1 + 1))
    return {p for p in want if p < HW and not any(p0 <= p < q for p0, q in runs)}


def check_run_logits(c, runs, ref_bound, what, idx=None, chunk_rows=None, stale=True):
    HW = int(np.prod(c['ar'].block_size[:2]))
    got = run_logits(c, runs, heads_behind(runs, HW), idx, chunk_rows, stale)
    assert got, (what, runs)
    rows = slice(None) if idx is None else np.asarray(idx)
    e_ref, e_path = [], []
    for i, lg in sorted(got.items()):
        for d, v in enumerate(c['vocab']):
            e_ref.append(np.abs(lg[:, d, :v].astype(np.float64) - c['ref'][rows, i, d, :v]).ravel())
            e_path.append(np.abs(lg[:, d, :v] - c['stepped'][rows, i, d, :v]).ravel())
    e_ref, e_path = np.concatenate(e_ref), np.concatenate(e_path)
    print('kept runs %s, runs %s: %d positions compared, vs the reference max %.4f mean %.5f, vs the stepped sequence max %.5f'
          % (what, runs, len(got), e_ref.max(), e_ref.mean(), e_path.max()))
    assert e_ref.max() < ref_bound[0] and e_ref.mean() < ref_bound[1], (what, runs)
    assert e_path.max() < PC.PATH_LOGIT, (what, runs)
    return got


def tiny_runs(HW=16):
    return [[(1, 3)], [(2, HW - 1)], [(1, 3), (5, 9)]]


def check_chunked(c, ref_bound):
    """tiny model, 5 images, the run (2, 15) of 13 tokens per image: 65 rows unchunked; fwd.chunk_rows = 30: chunks of 2 + 2 + 1 images;
    13: one image per chunk; 5: less than one run -- one image per chunk all the same.  All of them are GEMMs of at most 128 rows, one
    regime (csrc/gemm.hip: rq_gemm_pick_tile), and a row's attention does not know its chunk: the logits are equal bit for bit"""
    n = c['codes'].shape[0]
    idx = np.arange(5) % n
    base = check_run_logits(c, [(2, 15)], ref_bound, 'unchunked', idx=idx)
    for rows in (30, 13, 5):
        got = check_run_logits(c, [(2, 15)], ref_bound, f'fwd.chunk_rows = {rows}', idx=idx, chunk_rows=rows)
        assert sorted(got) == sorted(base)
        for i in base:
            assert np.array_equal(got[i].view(np.uint32), base[i].view(np.uint32)), f'fwd.chunk_rows = {rows}: logits differ in bits'


# ------------------------------------------------------------------------------------------------ 2. sampling inside the mode
def masks(H, W, device):
    """(H, W) keep masks and a start_loc each.  left: columns w < W / 2 kept (a run of W / 2 in front of every row's drawn half); band:
    rows 0 and 2 kept, rows 1 and 3 drawn (runs of W positions); start: start_loc = (1, 1) with the two positions behind it kept -- the
    run [1, W + 3) reaches across start_loc"""
    left = torch.zeros((H, W), dtype=torch.bool, device=device)
    left[:, :W // 2] = True
    band = torch.zeros((H, W), dtype=torch.bool, device=device)
    band[0::2] = True
    start = torch.zeros(H * W, dtype=torch.bool, device=device)
    start[W + 1:W + 3] = True
    return {'left': (left, (0, 0)), 'band': (band, (0, 0)), 'start': (start.view(H, W), (1, 1))}


def check_forms_agree(device, name, seed=11):
    """inside kept_run_mode = 'one_pass', after a call that left other rows in the cache: graphs == use_graph=False == per-image tensors
    == return_log_probs(); seeds(): graphs == eager, and an image is drawn alike in another row of the batch; sample_guided(guidance_scale=1) == the first
    half of sample over the 2B rows; kept codes come back as given, fillers at drawn positions are not read"""
    ar, aux, cond, partial = PC.sampling_setup(device)
    ar.kept_run_mode = 'one_pass'
    B, H, W, D = partial.shape
    mask, start = masks(H, W, device)[name]
    n0 = start[0] * W + start[1]
    given = mask.view(H * W).clone()
    given[:n0] = True                                              # positions whose codes the call does not draw
    kw = dict(cond=cond, keep_mask=mask, start_loc=start, **SAMPLER)

    def run(fn):
        M.seed_all(seed)
        return fn()
    M.seed_all(3)
    ar.sample(torch.zeros_like(partial), aux, cond=cond, **SAMPLER)                     # (stale cache rows everywhere)
    base = run(lambda: ar.sample(partial, aux, **kw))
    flat, bflat = partial.view(B, H * W, D), base.view(B, H * W, D)
    assert torch.equal(bflat[:, given], flat[:, given]), 'kept codes were changed'
    assert int(base.min()) >= 0 and int(base.max()) < 500
    assert not torch.equal(bflat[:, ~given], flat[:, ~given]), 'nothing was drawn'
    filled = partial.clone()
    filled.view(B, H * W, D)[:, ~given] = M.OUT_OF_RANGE
    assert torch.equal(run(lambda: ar.sample(filled, aux, **kw)), base), 'codes at drawn positions were read'
    ar.use_graph = False
    try:
        eager = run(lambda: ar.sample(partial, aux, **kw))
    finally:
        ar.use_graph = True
    assert torch.equal(eager, base), 'use_graph=False != graphs'
    per = run(lambda: ar.sample(partial, aux, cond=cond, keep_mask=mask, start_loc=start, temperature=torch.ones(B, device=device),
                                top_k=torch.full((B,), SAMPLER['top_k'], dtype=torch.long, device=device),
                                top_p=torch.full((B,), SAMPLER['top_p'], dtype=torch.float32, device=device)))
    assert torch.equal(per, base), 'per-image call != scalar call'
    with ar.return_log_probs():
        lp_codes, lp = run(lambda: ar.sample(partial, aux, **kw))
    assert torch.equal(lp_codes, base), 'return_log_probs() changed the codes'
    seeds = [101, 7, 55][:B]
    with ar.seeds(seeds):
        seeded = ar.sample(partial, aux, **kw)
        ar.use_graph = False
        try:
            seeded_eager = ar.sample(partial, aux, **kw)
        finally:
            ar.use_graph = True
        # (an image's draws follow its seed, not its row: the batch in reverse order under the reversed seeds)
    with ar.seeds(seeds[::-1]):
        flipped = ar.sample(partial.flip(0).contiguous(), aux, cond=cond.flip(0).contiguous(), keep_mask=mask, start_loc=start, **SAMPLER)
    assert torch.equal(seeded_eager, seeded), 'seeds(): use_graph=False != graphs'
    assert torch.equal(flipped.flip(0), seeded), 'seeds(): an image drawn in another row differs'
    assert torch.equal(seeded.view(B, H * W, D)[:, given], flat[:, given]) and not torch.equal(seeded, base)
    uncond = M.cond_for(C.RQT_TINY, B, device, seed=6)
    guided = run(lambda: ar.sample_guided(partial, aux, cond=cond, uncond=uncond, guidance_scale=1.0, keep_mask=mask, start_loc=start, **SAMPLER))
    twice = run(lambda: ar.sample(torch.cat([partial, partial]), aux, cond=torch.cat([cond, uncond]), keep_mask=mask, start_loc=start, **SAMPLER))
    assert torch.equal(guided, twice[:B]), 'sample_guided(1.0) != first half of sample over 2B rows'
    return ar, aux, cond, base, lp, given


def check_draws_see_the_runs(ar, aux, cond, codes, lp, given):
    """lp.model of the draws against log_probs(final codes) within ONEPASS_LOGP at every drawn code: the rows the passes wrote are the rows
    the later draws read.  NaN (model) and +0.0 (draw) at the kept positions (no head ran there)"""
    B, H, W, D = codes.shape
    model, draw = lp.model.view(B, H * W, D).cpu(), lp.draw.view(B, H * W, D).cpu()
    given = given.cpu()
    assert bool(torch.isnan(model[:, given]).all()), 'model log-probabilities at kept positions'
    assert bool((draw[:, given] == 0).all()) and not bool(torch.signbit(draw[:, given]).any()), 'draw log-probabilities at kept positions'
    full = ar.log_probs(codes, aux, cond=cond).view(B, H * W, D).cpu()
    err = float((model[:, ~given] - full[:, ~given]).abs().max())
    print('kept runs, model log-probabilities of the draws vs log_probs(codes): max %.5f' % err)
    assert err < ONEPASS_LOGP
    assert bool((draw[:, ~given] <= 0).all()) and bool(torch.isfinite(draw[:, ~given]).all())
    # (the comparison has teeth: under other kept codes the same draws have other log-probabilities)
    other = codes.clone()
    other.view(B, H * W, D)[:, given] = (other.view(B, H * W, D)[:, given] + 7) % 500
    shifted = ar.log_probs(other, aux, cond=cond).view(B, H * W, D).cpu()
    assert float((model[:, ~given] - shifted[:, ~given]).abs().max()) > ONEPASS_LOGP


# ------------------------------------------------------------------------------------------------ 3. the default
def check_default_untouched(device):
    """"masked.run_prefill" = 0 (set, or set to 1 and back) == a handle on which the option was never set; toggling captures nothing; an
    unmasked call before and after returns the same codes; the default mode is 'stepped'"""
    from rqvae.models.rqtransformer import RQTransformer
    assert RQTransformer(C.RQT_TINY).kept_run_mode == 'stepped'
    ar, aux, cond, partial = PC.sampling_setup(device)
    B, H, W, D = partial.shape
    mask, _ = masks(H, W, device)['left']

    def masked(a, x):
        M.seed_all(5)
        return a.sample(partial, x, cond=cond, keep_mask=mask, **SAMPLER)

    def unmasked(a, x):
        M.seed_all(6)
        return a.sample(torch.zeros_like(partial), x, cond=cond, **SAMPLER)
    never = masked(ar, aux)
    assert not hasattr(ar._eng(), '_kept_runs_one_pass')                  # the default never touches the option
    ar2, aux2, _, _ = PC.sampling_setup(device)
    plain = unmasked(ar2, aux2)
    eng = ar2._eng()
    eng.set_option('masked.run_prefill', 0)
    assert torch.equal(masked(ar2, aux2), never)
    n = eng.graph_captures()
    assert n >= 1 or torch.device(device).type == 'cpu'                   # (the host emulator captures nothing)
    eng.set_option('masked.run_prefill', 1)
    on = masked(ar2, aux2)
    assert torch.equal(on.view(B, H * W, D)[:, mask.view(-1)], partial.view(B, H * W, D)[:, mask.view(-1)])
    eng.set_option('masked.run_prefill', 0)
    assert torch.equal(masked(ar2, aux2), never)
    assert torch.equal(unmasked(ar2, aux2), plain)
    for mode in ('one_pass', 'stepped', 'one_pass', 'stepped'):
        ar2.kept_run_mode = mode
        assert torch.equal(masked(ar2, aux2), on if mode == 'one_pass' else never), mode
    assert eng.graph_captures() == n, 'toggling the option captured graphs again'
    assert ar2._eng() is eng


# ------------------------------------------------------------------------------------------------ 4. what stays stepped
def _on_off(ar, call):
    out = {}
    for mode in ('stepped', 'one_pass'):
        ar.kept_run_mode = mode
        M.seed_all(9)
        out[mode] = call()
    assert torch.equal(out['stepped'], out['one_pass'])
    return out['stepped']


def check_fallback_model(device, cfg, seed=43):
    """a handle the pass does not serve (RQAMD_KV=int8kv set by the caller, or a body head size other than 64): the option changes
    nothing, and step_run takes the steps themselves"""
    ar, aux = M.model(cfg, seed, device)
    H, W, D = cfg['block_size']
    B = 3
    cond = M.cond_for(cfg, B, device)
    partial = T(np.random.default_rng(seed + 1).integers(0, cfg['vocab_size'], (B, H, W, D)), device, torch.long)
    mask, _ = masks(H, W, device)['band']
    out = _on_off(ar, lambda: ar.sample(partial, aux, cond=cond, keep_mask=mask, **SAMPLER))
    assert not torch.equal(out, partial)
    eng, cbs = ar._eng(), ar._checked_codebooks(aux)
    lg = []
    for use_run in (False, True):
        eng.step_begin(partial, cond, cbs)
        eng.step_logits(0, -1)
        if use_run:
            eng.step_run(1, 5)
        else:
            for p in range(1, 5):
                eng.step_logits(p, -1)
        lg.append(eng.step_logits(5, 0).cpu().clone())
        eng.step_end()
    assert torch.equal(lg[0], lg[1]), 'step_run on a handle the pass does not serve != the steps themselves'


def check_fallback_shared(device, seed=44):
    """a shared_cond() call (text-conditioned tiny model, 2 prompts x 2 images) steps its kept runs whatever the option says"""
    cfg = C.RQT_TINY_TXT
    ar, aux = M.model(cfg, seed, device)
    H, W, D = cfg['block_size']
    cond = M.cond_for(cfg, 2, device)
    partial = T(np.random.default_rng(seed + 1).integers(0, cfg['vocab_size'], (4, H, W, D)), device, torch.long)
    mask, _ = masks(H, W, device)['band']

    def call():
        with ar.shared_cond(2):
            return ar.sample(partial, aux, cond=cond, keep_mask=mask, **SAMPLER)
    _on_off(ar, call)


def check_single_position_runs(device):
    """every other position kept: no run of two positions, the option changes nothing"""
    ar, aux, cond, partial = PC.sampling_setup(device)
    B, H, W, D = partial.shape
    mask = (torch.arange(H * W, device=device) % 2 == 0).view(H, W)
    _on_off(ar, lambda: ar.sample(partial, aux, cond=cond, keep_mask=mask, **SAMPLER))


# ------------------------------------------------------------------------------------------------ 5. errors
def check_errors(nat, device):
    """every refusal happens on the host, before anything is launched"""
    import pytest
    ar, aux, cond, partial = PC.sampling_setup(device, B=2)
    eng = ar._eng()
    cbs = ar._checked_codebooks(aux)
    HW = 16
    with pytest.raises(nat.RqamdError, match='step_begin'):
        eng.step_run(1, 3)                                                 # before step_begin
    eng.step_begin(partial, cond, cbs)
    with pytest.raises(nat.RqamdError, match='stands at step'):
        eng.step_run(1, 3)                                                 # at the wrong position (0)
    for p0, p1 in ((0, 3), (-1, 2), (1, HW), (1, HW + 4), (3, 3), (3, 2)):
        with pytest.raises(ValueError, match='rqt_step_run: positions'):
            eng.step_run(p0, p1)
    eng.step_logits(0, -1)
    with pytest.raises(nat.RqamdError, match='stands at step'):
        eng.step_run(2, 4)                                                 # at the wrong position (1)
    eng.step_run(1, 3)
    with pytest.raises(nat.RqamdError, match='stands at step'):
        eng.step_run(1, 3)                                                 # twice
    eng.step_logits(3, 0)
    with pytest.raises(nat.RqamdError, match='stands at step'):
        eng.step_run(3, 5)                                                 # after a head step of p0
    for d in range(1, 4):
        eng.step_logits(3, d)
    eng.step_run(4, HW - 1)                                                # the longest run there is
    eng.step_logits(HW - 1, 0)
    eng.step_end()
    with pytest.raises(nat.RqamdError, match='step_begin'):
        eng.step_run(1, 3)                                                 # after step_end
    for bad in (2, -1):
        with pytest.raises(ValueError, match='masked.run_prefill'):
            eng.set_option('masked.run_prefill', bad)
    ar.kept_run_mode = 'x'
    with pytest.raises(ValueError, match='kept_run_mode'):
        ar.sample(partial, aux, cond=cond, start_loc=(1, 0))
    with pytest.raises(ValueError, match='kept_run_mode'):
        ar.sample_guided(partial, aux, cond=cond, start_loc=(1, 0))
    ar.kept_run_mode = 'stepped'
