"""Shared by tests/test_emu_soft_loss.py (host emulator) and tests/test_gpu_soft_loss.py (MI355X): the checks of the soft-target cross
entropy -- rqamd_soft_ce (soft_ce_kernel alone), compute_loss / compute_codebook_loss(use_soft_target=True), rqamd_rqt_soft_loss and
RQTransformer.soft_target_loss in both forms (soft targets given / formed in the engine from the features) -- and the inputs of the
fixture tests/golden/rqt_tiny_soft_loss.npz (tests/golden/make_golden_soft_loss.py imports this module for them: nothing here may
import the package at module level).

Bounds
  KERNEL     the kernel alone against ref64() (the reference's formula, rqvae/optimizer/loss.py:68-76, in float64, the 1e-7 included), as
             |got - want| / max(1, |want|): the loss is a difference of two sums of the size of sum(t) * |logit|, so its fp32 error scales
             with the loss.  Twice the largest value measured (KERNEL_MEASURED, emulator / MI355X).
  DERIVED    engine against the reference's per-code loss of the fixture: sum t = 1, so logits within e of the reference's move the loss by
             at most 2 e; with the logits bounds of the one-pass tests (0.03 max / 0.0045 mean) that is 0.06 max and 0.009 mean, and 0.009
             for the scalar and per-depth means.  Derived, never measured.
  PAIR       form (b) against form (a) of the same call: the same logits rows and the same target logits; (a) rounds every target
             probability (exp2 approximation, division) before the sum, (b) forms one quotient at the end.  Twice the measured value.
  ONEHOT     form (a) with one-hot targets against -log_probs: log(S + 1e-7) - log(S) <= 1e-7 plus the rounding of two reductions of the
             same rows; twice the measured value and never above KERNEL + 1e-7.
  WIDE       RQT_WIDE and the fp16 engine against ref64() of the one-pass logits and get_soft_codes output of the same inputs (GPU only)."""
import numpy as np
import torch

from oracle import configs as C

MODEL_SEED, CB_SEED, Z_SEED, STOCHASTIC_SEED = 41, 51, 52, 53
TEMP = 0.1
POS = [0, 5, 10, 15]                  # spatial positions (of 16) whose logits and soft codes the fixture stores

# largest |got - want| / max(1, |want|) of case 1 over every shape, target and logits kind: emulator (host libm) / MI355X
KERNEL_MEASURED = {'emu': 3.93e-07, 'gpu': 3.93e-07}
KERNEL_BOUND = 2 * max(KERNEL_MEASURED.values())
DERIVED_MAX, DERIVED_MEAN = 2 * 0.03, 2 * 0.0045
PAIR_MEASURED = {'emu': 1.44e-06, 'gpu': 1.44e-06}      # max |form (b) - form (a)| over the per-code losses of the fixture's inputs
PAIR_BOUND = 2 * max(PAIR_MEASURED.values())
ONEHOT_MEASURED = {'emu': 4.77e-07, 'gpu': 4.77e-07}
ONEHOT_BOUND = min(2 * max(ONEHOT_MEASURED.values()), KERNEL_BOUND + 1e-7)
CHUNK_BOUND = 2 * 0.02                # between chunkings: 0.02 per logit (the one-pass tests' bound between GEMM tile choices), twice that per loss
WIDE_MEASURED = {'wide_a': 2.15e-07, 'wide_b': 2.17e-07, 'amp_a': 2.09e-07, 'amp_b': 2.25e-07}      # MI355X, relative as KERNEL
OBSERVED = {}


def note(key, value):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(value))
    print('soft loss, observed %s: %.3e' % (key, OBSERVED[key]))
    return value


# ------------------------------------------------------------------------------------------------ inputs of the fixture
def codebook():
    return (0.1 * np.random.default_rng(CB_SEED).standard_normal((500, 64))).astype(np.float32)


def features():
    return (0.15 * np.random.default_rng(Z_SEED).standard_normal((2, 4, 4, 64))).astype(np.float32)


def cond(cfg):
    return np.random.default_rng(54).integers(0, cfg['vocab_size_cond'], (2, max(cfg['block_size_cond'], 1)))


def ref64(x, t):
    """soft_target_cross_entropy(reduction='none') (rqvae/optimizer/loss.py:68-76) in float64"""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    with np.errstate(all='ignore'):
        m = x.max(-1, keepdims=True)
        logp = x - m - np.log(np.exp(x - m).sum(-1, keepdims=True) + 1e-7)
        return (-t * logp).sum(-1)


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
SHAPES = ((1, 500, None), (3, 501, 501), (5, 16384, None), (257, 1000, None), (4, 500, 512))      # (rows, V, leading dimension)
TARGETS = ('softmax', 'positive', 'onehot', 'zero_row')
LOGITS = ('normal', 'outlier', 'constant')


def kernel_inputs(rows, V, tkind, lkind, seed):
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
    if lkind == 'outlier':
        x[rows // 2, V // 3] += 80.0
    elif lkind == 'constant':
        x[rows // 2, :] = 1.25
    if tkind in ('softmax', 'zero_row'):
        n = rng.standard_normal((rows, V))
        t = np.exp(n - n.max(-1, keepdims=True))
        t = (t / t.sum(-1, keepdims=True)).astype(np.float32)
        if tkind == 'zero_row':
            t[rows // 2, :] = 0.0
    elif tkind == 'positive':
        t = (rng.random((rows, V)) * (6.0 / V)).astype(np.float32)       # unnormalised: sums of about 3
    else:
        t = np.zeros((rows, V), np.float32)
        t[np.arange(rows), rng.integers(0, V, rows)] = 1.0
    return x, t


def strided(a, ld, dev):
    """the (rows, V) matrix as a column slice of a (rows, ld) one (NaN outside), or contiguous"""
    if ld is None or ld == a.shape[1]:
        return torch.from_numpy(a).to(dev)
    wide = torch.full((a.shape[0], ld), float('nan'), dtype=torch.float32)
    wide[:, :a.shape[1]] = torch.from_numpy(a)
    return wide.to(dev)[:, :a.shape[1]]


def check_kernel(nat, dev, where):
    worst = 0.0
    for si, (rows, V, ld) in enumerate(SHAPES):
        for ti, tkind in enumerate(TARGETS):
            for li, lkind in enumerate(LOGITS):
                x, t = kernel_inputs(rows, V, tkind, lkind, 1000 + 100 * si + 10 * ti + li)
                got = nat.soft_ce(strided(x, ld, dev), strided(t, ld, dev)).cpu().numpy()
                want = ref64(x, t)
                err = rel_err(got, want).max()
                worst = max(worst, err)
                if tkind == 'zero_row':
                    assert got[rows // 2] == 0.0, (rows, V, lkind, got[rows // 2])
                assert np.isfinite(got).all()
    note('kernel ' + where, worst)
    assert worst <= KERNEL_BOUND, (worst, KERNEL_BOUND)
    # the unaligned base: rows of a 16-byte aligned matrix taken from column 1 on (scalar loads)
    x, t = kernel_inputs(3, 501, 'softmax', 'normal', 7)
    got = nat.soft_ce(torch.from_numpy(x).to(dev)[:, 1:], torch.from_numpy(t).to(dev)[:, 1:]).cpu().numpy()
    assert rel_err(got, ref64(x[:, 1:], t[:, 1:])).max() <= KERNEL_BOUND
    return worst


def check_kernel_nonfinite(nat, dev):
    for rows, V, ld in ((3, 500, None), (3, 501, 501)):                  # 16-byte loads / scalar loads
        x, t = kernel_inputs(rows, V, 'softmax', 'normal', 5)
        t[:, 7] = 0.0
        x[0, 3] = np.nan                                                # a NaN logit: NaN
        x[1, 7] = -np.inf                                               # -inf under a zero target: 0 * -inf = NaN
        x[2, 9] = -np.inf                                               # -inf under a positive target: +inf
        assert t[2, 9] > 0
        got = nat.soft_ce(strided(x, ld, dev), strided(t, ld, dev)).cpu().numpy()
        want = ref64(x, t)
        assert np.isnan(want[0]) and np.isnan(want[1]) and want[2] == np.inf
        assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == np.inf, got


# ------------------------------------------------------------------------------------------------ models on the fixture's inputs
class Aux:
    """model_aux of the tests: the quantiser of an RQVAE (shared codebook of the fixture) and its get_soft_codes"""

    def __init__(self, cb, dev, dim=64, hw=4, depth=4):
        from rqvae.models.rqvae.quantizations import RQBottleneck
        self.quantizer = RQBottleneck(latent_shape=(hw, hw, dim), code_shape=(hw, hw, depth), n_embed=cb.shape[0], shared_codebook=True)
        with torch.no_grad():
            self.quantizer.codebooks[0].weight[:-1] = torch.from_numpy(cb)
        self.quantizer = self.quantizer.to(dev).eval()

    def get_soft_codes(self, z, temp=1.0, stochastic=False):
        return self.quantizer.get_soft_codes(z, temp=temp, stochastic=stochastic)


def model(cfg, dev, seed=MODEL_SEED):
    import oracle
    from rqvae.models.rqtransformer import RQTransformer
    ar = RQTransformer(cfg).eval()
    ar.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqt_param_shapes(cfg), seed, cfg).items()}, strict=True)
    return ar.to(dev)


_SHARED = {}


def tiny(dev, golden):
    """the tiny model, the fixture's inputs and what several checks need of them, computed once per device"""
    key = str(dev)
    if key not in _SHARED:
        g = golden('rqt_tiny_soft_loss.npz')
        assert np.array_equal(g['z'], features()) and float(g['temp']) == np.float32(TEMP)
        aux = Aux(codebook(), dev)
        ar = model(C.RQT_TINY, dev)
        z = torch.from_numpy(g['z']).to(dev)
        soft, codes = aux.get_soft_codes(z, temp=TEMP)
        assert np.array_equal(codes.cpu().numpy(), g['a_codes'])          # the engine's argmin codes are the reference's
        cnd = torch.from_numpy(g['cond'].astype(np.int64)).to(dev)
        loss_a = ar.soft_target_loss(codes, aux, cond=cnd, soft_targets=soft)
        _SHARED[key] = dict(g=g, aux=aux, ar=ar, z=z, soft=soft, codes=codes, cond=cnd, loss_a=loss_a)
    return _SHARED[key]


def derived(got, g, tag, what):
    got = got.cpu().numpy()
    err = np.abs(got - g[tag + 'loss'])
    print('soft loss, %s: per-code max err %.4f mean %.5f; scalar %.5f; per depth %s' % (
        what, err.max(), err.mean(), abs(got.mean() - float(g[tag + 'loss_mean'])), np.abs(got.mean((0, 1, 2)) - g[tag + 'loss_depth'])))
    assert got.dtype == np.float32 and got.shape == g[tag + 'loss'].shape
    assert err.max() < DERIVED_MAX and err.mean() < DERIVED_MEAN, what
    assert abs(got.mean() - float(g[tag + 'loss_mean'])) < DERIVED_MEAN, what
    assert np.abs(got.mean((0, 1, 2)) - g[tag + 'loss_depth']).max() < DERIVED_MEAN, what


# ------------------------------------------------------------------------------------------------ 2. compute_loss / compute_codebook_loss
def check_compute_loss(dev, golden):
    s = tiny(dev, golden)
    g, ar = s['g'], s['ar']
    for tag in ('a_', 's_'):
        x, t = g[tag + 'logits_pos'], g[tag + 'soft_pos']                 # (2, 4 positions, 4, 500) of the reference
        want = ref64(x, t)
        tx, tt = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
        got = ar.compute_loss(tx, tt, use_soft_target=True)
        assert got.dim() == 0 and got.dtype == torch.float32
        assert abs(float(got) - want.mean()) <= KERNEL_BOUND * max(1.0, want.mean())
        depth = ar.compute_codebook_loss(tx, tt, use_soft_target=True).cpu().numpy()
        assert depth.shape == (4,)
        assert rel_err(depth, want.reshape(-1, 4).mean(0)).max() <= KERNEL_BOUND
        # float64 logits (computed in fp32), and non-contiguous views of both
        got64 = ar.compute_loss(tx.double(), tt, use_soft_target=True)
        assert got64.dtype == torch.float32 and float(got64) == float(got)
        wide_x, wide_t = torch.zeros((2, 4, 4, 1000), device=dev), torch.zeros((2, 4, 4, 1000), device=dev)
        wide_x[..., ::2], wide_t[..., ::2] = tx, tt
        assert not wide_x[..., ::2].is_contiguous()
        assert float(ar.compute_loss(wide_x[..., ::2], wide_t[..., ::2], use_soft_target=True)) == float(got)
        perm = ar.compute_codebook_loss(tx.permute(1, 0, 2, 3), tt.permute(1, 0, 2, 3), use_soft_target=True).cpu().numpy()
        assert rel_err(perm, depth).max() <= 1e-6                         # (another order of the rows in the mean)
        # a flat (rows, V) call
        assert float(ar.compute_loss(tx.reshape(-1, 500), tt.reshape(-1, 500), use_soft_target=True)) == float(got)
    need_grad = tx.clone().requires_grad_(True)
    for fn in (ar.compute_loss, ar.compute_codebook_loss):
        try:
            fn(need_grad, tt, use_soft_target=True)
        except NotImplementedError as e:
            assert 'grad' in str(e)
        else:
            raise AssertionError('logits that require grad were accepted')
    # the hard-target paths are what they were
    hard = torch.from_numpy(g['a_codes'].astype(np.int64).reshape(2, 16, 4)[:, POS]).to(dev)
    want = torch.nn.functional.cross_entropy(tx.reshape(-1, 500), hard.reshape(-1))
    assert float(ar.compute_loss(tx, hard)) == float(want)


# ------------------------------------------------------------------------------------------------ 3. / 4. / 5. the engine forms
def check_form_a(dev, golden):
    s = tiny(dev, golden)
    derived(s['loss_a'], s['g'], 'a_', 'form (a), argmin codes')
    # the engine's soft codes at the stored positions are the reference's
    soft_pos = s['soft'].cpu().numpy().reshape(2, 16, 4, 500)[:, POS]
    assert np.abs(soft_pos - s['g']['a_soft_pos']).max() < 1e-5


def check_form_b(dev, golden, where):
    s = tiny(dev, golden)
    g, ar, aux = s['g'], s['ar'], s['aux']
    loss_b = ar.soft_target_loss(s['codes'], aux, cond=s['cond'], z_e=s['z'], temp=TEMP)
    derived(loss_b, g, 'a_', 'form (b), argmin codes')
    diff = float((loss_b - s['loss_a']).abs().max())
    note('pair ' + where, diff)
    assert diff <= PAIR_BOUND, (diff, PAIR_BOUND)
    # stochastic codes of the reference: the residual follows the GIVEN codes
    sc = torch.from_numpy(g['s_codes'].astype(np.int64)).to(dev)
    loss_s = ar.soft_target_loss(sc, aux, cond=s['cond'], z_e=s['z'], temp=TEMP)
    derived(loss_s, g, 's_', 'form (b), stochastic codes')
    assert float((loss_s - loss_b).abs().max()) > 0.1                    # (and they are other codes: another loss)
    return loss_b


def check_onehot(dev, golden, where):
    s = tiny(dev, golden)
    ar, aux, codes = s['ar'], s['aux'], s['codes']
    onehot = torch.nn.functional.one_hot(codes, 500).to(torch.float32)
    got = ar.soft_target_loss(codes, aux, cond=s['cond'], soft_targets=onehot)
    lp = ar.log_probs(codes, aux, cond=s['cond'])
    diff = float((got + lp).abs().max())
    note('onehot ' + where, diff)
    assert diff <= ONEHOT_BOUND, (diff, ONEHOT_BOUND)


# ------------------------------------------------------------------------------------------------ 6. chunking
def check_chunked(dev, golden, full=True):
    """full = False (the emulator, half a minute per call on 7 images): without the repeated log_probs calls and the one-group sub-chunks"""
    s = tiny(dev, golden)
    g, ar, aux = s['g'], s['ar'], s['aux']
    idx = np.arange(7) % 2
    tidx = torch.from_numpy(idx).to(dev)
    codes, cnd, z, soft = s['codes'][tidx], s['cond'][tidx], s['z'][tidx], s['soft'][tidx]
    eng = ar._eng()
    base_lp = ar.log_probs(codes, aux, cond=cnd)
    eng.set_option('fwd.logits_bytes', 48 << 20)                          # the default, given explicitly: the same bits
    assert torch.equal(ar.log_probs(codes, aux, cond=cnd), base_lp)
    whole_a = ar.soft_target_loss(codes, aux, cond=cnd, soft_targets=soft)
    whole_b = ar.soft_target_loss(codes, aux, cond=cnd, z_e=z, temp=TEMP)
    want = {k: g[k] for k in ('a_loss_mean', 'a_loss_depth')}
    want['a_loss'] = g['a_loss'][idx]
    try:
        eng.set_option('fwd.logits_bytes', 3 * 4 * 500 * 4)               # 3 depth groups of V = 500 per classifier sub-chunk
        for rows in (3 * 16, 20):                                         # body chunks of 3 + 3 + 1 images; one image, head sub-chunks of 5 = 3 + 2
            eng.set_option('fwd.chunk_rows', rows)
            for what, whole, kw in (('a', whole_a, dict(soft_targets=soft)), ('b', whole_b, dict(z_e=z, temp=TEMP))):
                got = ar.soft_target_loss(codes, aux, cond=cnd, **kw)
                err = np.abs(got.cpu().numpy() - want['a_loss'])
                print('soft loss chunked, form (%s), fwd.chunk_rows %d: max err %.4f mean %.5f, to the unchunked call %.5f' % (
                    what, rows, err.max(), err.mean(), float((got - whole).abs().max())))
                assert err.max() < DERIVED_MAX and err.mean() < DERIVED_MEAN
                assert float((got - whole).abs().max()) < CHUNK_BOUND
            if full:
                lp = ar.log_probs(codes, aux, cond=cnd)
                assert float((lp - base_lp).abs().max()) < CHUNK_BOUND
        for bad in (0, -5):
            try:
                eng.set_option('fwd.logits_bytes', bad)
            except ValueError:
                pass
            else:
                raise AssertionError('fwd.logits_bytes = %d accepted' % bad)
        if full:
            eng.set_option('fwd.logits_bytes', 1)                         # below one depth group: one depth group
            got = ar.soft_target_loss(codes, aux, cond=cnd, z_e=z, temp=TEMP)
            assert float((got - whole_b).abs().max()) < CHUNK_BOUND
    finally:
        eng.set_option('fwd.logits_bytes', 48 << 20)
        eng.set_option('fwd.chunk_rows', 4096)
    if full:
        assert torch.equal(ar.log_probs(codes, aux, cond=cnd), base_lp)


# ------------------------------------------------------------------------------------------------ 7. text-conditioned
def check_txt(dev, golden):
    s = tiny(dev, golden)
    g, aux = s['g'], s['aux']
    art = model(C.RQT_TINY_TXT, dev)
    cnd = torch.from_numpy(g['t_cond'].astype(np.int64)).to(dev)
    lp, cond_lp = art.log_probs(s['codes'], aux, cond=cnd)
    for kw in (dict(soft_targets=s['soft']), dict(z_e=s['z'], temp=TEMP)):
        loss, cl = art.soft_target_loss(s['codes'], aux, cond=cnd, **kw)
        assert torch.equal(cl, cond_lp)                                   # same kernels over the same rows
        derived(loss, g, 't_', 'text-conditioned, ' + ', '.join(kw))
    try:
        art.soft_target_loss(s['codes'], aux, soft_targets=s['soft'])
    except ValueError:
        pass
    else:
        raise AssertionError('a text-conditioned model without cond was accepted')


# ------------------------------------------------------------------------------------------------ 8. refusals
def check_refusals(nat, dev, golden):
    import ctypes
    import pytest
    s = tiny(dev, golden)
    ar, aux, codes, soft, z = s['ar'], s['aux'], s['codes'], s['soft'], s['z']
    with pytest.raises(ValueError):
        ar.soft_target_loss(codes, aux, soft_targets=soft, z_e=z)
    with pytest.raises(ValueError):
        ar.soft_target_loss(codes, aux)
    with pytest.raises(ValueError):
        ar.soft_target_loss(codes, aux, soft_targets=soft[..., :499])
    with pytest.raises(ValueError):
        ar.soft_target_loss(codes, aux, z_e=z, temp=0.0)
    with pytest.raises(ValueError):
        ar.soft_target_loss(codes, aux, z_e=z, temp=float('nan'))
    tup = model(C.RQT_TINY_TUPLE, dev)
    with pytest.raises(NotImplementedError):
        tup.soft_target_loss(codes % 200, None, soft_targets=soft)
    with pytest.raises(NotImplementedError):
        tup.soft_target_loss(codes % 200, aux, z_e=z, temp=TEMP)
    # at the ABI: the error code, rqamd_last_error, and nothing written
    L = nat.lib()
    eng = ar._eng()
    out = torch.full((2, 4, 4, 4), -7.0, dtype=torch.float32, device=dev)
    cbs = nat._ptr_array(aux.quantizer.codebook_list())
    nrm = nat._ptr_array(aux.quantizer._norm_list())
    st = nat.stream_of(out)
    p = nat.ptr
    calls = {
        'null handle': lambda: L.rqamd_rqt_soft_loss(None, p(codes), None, 2, cbs, p(soft), None, None, 1.0, p(out), None, st),
        'null codes': lambda: L.rqamd_rqt_soft_loss(eng._h, None, None, 2, cbs, p(soft), None, None, 1.0, p(out), None, st),
        'null loss_out': lambda: L.rqamd_rqt_soft_loss(eng._h, p(codes), None, 2, cbs, p(soft), None, None, 1.0, None, None, st),
        'neither': lambda: L.rqamd_rqt_soft_loss(eng._h, p(codes), None, 2, cbs, None, None, None, 1.0, p(out), None, st),
        'both': lambda: L.rqamd_rqt_soft_loss(eng._h, p(codes), None, 2, cbs, p(soft), p(z), nrm, 1.0, p(out), None, st),
        'z without norms': lambda: L.rqamd_rqt_soft_loss(eng._h, p(codes), None, 2, cbs, None, p(z), None, 1.0, p(out), None, st),
        'temp 0': lambda: L.rqamd_rqt_soft_loss(eng._h, p(codes), None, 2, cbs, None, p(z), nrm, 0.0, p(out), None, st),
        'temp nan': lambda: L.rqamd_rqt_soft_loss(eng._h, p(codes), None, 2, cbs, None, p(z), nrm, float('nan'), p(out), None, st),
        'batch 0': lambda: L.rqamd_rqt_soft_loss(eng._h, p(codes), None, 0, cbs, p(soft), None, None, 1.0, p(out), None, st),
        'cond_logp without a prefix': lambda: L.rqamd_rqt_soft_loss(eng._h, p(codes), None, 2, cbs, p(soft), None, None, 1.0, p(out), p(out), st),
        'soft_ce null logits': lambda: L.rqamd_soft_ce(None, 500, p(soft), 500, 4, 500, p(out), st),
        'soft_ce null targets': lambda: L.rqamd_soft_ce(p(soft), 500, None, 500, 4, 500, p(out), st),
        'soft_ce null out': lambda: L.rqamd_soft_ce(p(soft), 500, p(soft), 500, 4, 500, None, st),
        'soft_ce ld < vocab': lambda: L.rqamd_soft_ce(p(soft), 499, p(soft), 500, 4, 500, p(out), st),
        'soft_ce vocab 0': lambda: L.rqamd_soft_ce(p(soft), 500, p(soft), 500, 4, 0, p(out), st),
    }
    for what, call in calls.items():
        with nat.on_device_of(out):
            rc = call()
        assert rc == -1, (what, rc)
        msg = L.rqamd_last_error().decode()
        assert ('soft_loss' in msg or 'soft_ce' in msg), (what, msg)
    tup_eng = tup._eng()
    with nat.on_device_of(out):
        rc = L.rqamd_rqt_soft_loss(tup_eng._h, p(codes), None, 2, cbs, p(soft), None, None, 1.0, p(out), None, st)
    assert rc == -2 and 'one vocabulary' in L.rqamd_last_error().decode()
    if out.is_cuda:
        torch.cuda.synchronize(dev)
    assert bool((out == -7.0).all()), 'a refused call wrote its output'
    assert ctypes.c_int(L.rqamd_soft_ce(None, 0, None, 0, 0, 500, None, st)).value == 0       # no rows: nothing to do
