"""MI355X checks of the soft-target cross entropy (rqamd_soft_ce, compute_loss(use_soft_target=True), rqamd_rqt_soft_loss /
RQTransformer.soft_target_loss): the cases of tests/soft_loss_cases.py, which the host emulator runs as well
(tests/test_emu_soft_loss.py), on the real kernels, plus the wide model and the fp16 engine."""
import numpy as np
import pytest
import torch

import oracle
from oracle import configs as C
import soft_loss_cases as SL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def nat():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from rqvae import _native
    _native.lib()
    yield _native
    SL._SHARED.pop(DEV, None)
    torch.cuda.empty_cache()


def test_soft_ce_kernel_against_float64(nat):
    """case 1: soft_ce_kernel alone, 5 shapes x 4 kinds of targets x 3 kinds of logits, against float64 of the reference's formula.
    Largest |got - want| / max(1, |want|): 3.93e-07 in the emulator, 3.93e-07 on the MI355X (soft_loss_cases.KERNEL_MEASURED); the bound is
    twice the larger, 7.86e-07."""
    SL.check_kernel(nat, DEV, 'gpu')


def test_soft_ce_kernel_nonfinite(nat):
    SL.check_kernel_nonfinite(nat, DEV)


def test_compute_loss_soft_target(nat, golden):
    SL.check_compute_loss(DEV, golden)


def test_soft_target_loss_targets_given(nat, golden):
    SL.check_form_a(DEV, golden)


def test_soft_target_loss_from_features(nat, golden):
    """case 4; form (b) against form (a): 1.44e-06 in the emulator and on the MI355X (soft_loss_cases.PAIR_MEASURED), bound 2.88e-06"""
    SL.check_form_b(DEV, golden, 'gpu')


def test_soft_target_loss_onehot_is_log_probs(nat, golden):
    SL.check_onehot(DEV, golden, 'gpu')


def test_soft_target_loss_chunked(nat, golden):
    SL.check_chunked(DEV, golden)


def test_soft_target_loss_text_conditioned(nat, golden):
    SL.check_txt(DEV, golden)


def test_soft_target_loss_refusals(nat, golden):
    SL.check_refusals(nat, DEV, golden)


# ------------------------------------------------------------------------------------------------ 9. GPU only
def _against_host_route(ar, aux, codes, cond, z, temp, amp, keys):
    """both forms against float64 of the reference's formula over the one-pass forward logits and the get_soft_codes output of the
    same inputs (two entry points that predate the soft loss)"""
    soft, qcodes = aux.get_soft_codes(z, temp=temp)
    assert torch.equal(qcodes, codes)
    ar.forward_mode = 'one_pass'
    logits = ar(codes, aux, cond=cond, amp=amp)
    want = SL.ref64(logits.cpu().numpy(), soft.cpu().numpy())
    top = soft.amax(-1)
    print('host route: loss %.4f, largest target probability median %.3f' % (want.mean(), float(top.median())))
    for key, kw in zip(keys, (dict(soft_targets=soft), dict(z_e=z, temp=temp))):
        got = ar.soft_target_loss(codes, aux, cond=cond, amp=amp, **kw).cpu().numpy()
        err = SL.rel_err(got, want).max()
        SL.note(key, err)
        assert err <= 2 * SL.WIDE_MEASURED[key], (key, err)


def test_soft_target_loss_wide_model(nat):
    """RQT_WIDE (E 1536, V 16384, input_embed_dim 256, 2 + 1 layers), 2 images.  Largest |got - want| / max(1, |want|) on the MI355X:
    2.15e-07 (targets given) and 2.17e-07 (targets from the features), soft_loss_cases.WIDE_MEASURED; the bounds are twice those."""
    from rqvae.models.rqtransformer import RQTransformer
    cfg = C.RQT_WIDE
    ar = RQTransformer(cfg).eval()
    sd = ar.state_dict()
    with torch.no_grad():
        for k, shp in oracle.rqt_param_shapes(cfg).items():
            sd[k].copy_(torch.from_numpy(oracle.weights.make_tensor(k, shp, 61)))
    ar = ar.to(DEV)
    rng = np.random.default_rng(62)
    cb = (0.1 * rng.standard_normal((16384, 256))).astype(np.float32)
    z = torch.from_numpy((0.15 * rng.standard_normal((2, 8, 8, 256))).astype(np.float32)).to(DEV)
    aux = SL.Aux(cb, DEV, dim=256, hw=8, depth=4)
    codes = aux.quantizer.get_codes_only(z)
    cond = torch.tensor([[3], [900]], device=DEV)
    _against_host_route(ar, aux, codes, cond, z, 0.5, False, ('wide_a', 'wide_b'))


def test_soft_target_loss_fp16_engine(nat, golden):
    """the tiny model with amp=True, on the fp16 build of the engine: 2.09e-07 / 2.25e-07 measured (WIDE_MEASURED), bounds twice those"""
    s = SL.tiny(DEV, golden)
    _against_host_route(s['ar'], s['aux'], s['codes'], s['cond'], s['z'], SL.TEMP, True, ('amp_a', 'amp_b'))
    s['ar'].forward_mode = 'stepped'
