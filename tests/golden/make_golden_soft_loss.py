#!/usr/bin/env python
"""Generate tests/golden/rqt_tiny_soft_loss.npz -- the soft-target cross entropy of stage 2 -- by running the REFERENCE ITSELF on the
CPU, the way make_golden.py does for the other fixtures (same stub, same seeded weights):

    soft_codes, codes = RQBottleneck.get_soft_codes(z, temp, stochastic)      (quantizations.py:371-400)
    logits = RQTransformer(codes, model_aux, cond)                             (transformers.py:113-188)
    soft_target_cross_entropy(logits, soft_codes, reduction='none')           (rqvae/optimizer/loss.py:68-84)
    compute_loss / compute_codebook_loss(logits, soft_codes, use_soft_target=True)   (transformers.py:371-410)

    python tests/golden/make_golden_soft_loss.py

Needs the reference checkout next to the build (see make_golden.py).  Three sets: 'a_' RQT_TINY with the argmin codes, 's_' the same with
stochastic codes (torch.manual_seed; the codes are not the argmin), 't_' RQT_TINY_TXT with the argmin codes.  Each stores codes and the
reference's losses in full, logits and soft codes at four positions only; the codebook and the features are regenerated from their
seeds by tests/soft_loss_cases.py (the features are stored as well).
"""
import os
import sys

import numpy as np

import make_golden as mg          # the reference behind its omegaconf stub, ref_rqt(), CodebookAux, save()

sys.path.insert(0, os.path.dirname(mg.HERE))
import soft_loss_cases as SL      # noqa: E402  (tests/soft_loss_cases.py: seeds, scales, stored positions)

from rqvae.models.rqvae.quantizations import RQBottleneck  # noqa: E402  (reference)
from rqvae.optimizer.loss import soft_target_cross_entropy  # noqa: E402  (reference)

torch = mg.torch
C = mg.C


def ref_quantizer(cb):
    q = RQBottleneck(latent_shape=[4, 4, 64], code_shape=[4, 4, 4], n_embed=cb.shape[0], shared_codebook=True).eval()
    w = q.codebooks[0].weight.data
    assert tuple(w.shape) == (cb.shape[0] + 1, cb.shape[1])
    w[:-1] = torch.from_numpy(cb)
    return q


def one_set(m, q, cb, z, cond, stochastic, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    soft, codes = q.get_soft_codes(torch.from_numpy(z), temp=SL.TEMP, stochastic=stochastic)
    logits = m(codes, mg.CodebookAux(cb), cond=torch.from_numpy(cond))
    logits = logits[0] if isinstance(logits, tuple) else logits
    per_code = soft_target_cross_entropy(logits, soft, reduction='none')
    loss = m.compute_loss(logits, soft, use_soft_target=True)
    depth = m.compute_codebook_loss(logits, soft, use_soft_target=True)
    assert abs(float(per_code.mean()) - float(loss)) < 1e-5
    (B, H, W, D, V) = logits.shape
    flat = lambda t: t.numpy().reshape(B, H * W, D, V)[:, SL.POS]
    argmin = q.get_soft_codes(torch.from_numpy(z), temp=SL.TEMP, stochastic=False)[1]
    top = soft.numpy().max(-1)
    print(f'  stochastic={stochastic}: loss {float(loss):.4f}, per depth {np.round(depth.numpy(), 4)}; codes differ from the argmin in '
          f'{int((codes != argmin).sum())} of {codes.numel()}; largest target probability per row: median {np.median(top):.3f}, '
          f'range {top.min():.3f} .. {top.max():.3f}; per depth median {np.round(np.median(top.reshape(-1, D), 0), 3)}')
    # the targets are genuinely soft (a near one-hot fixture would not tell the soft loss from the hard one)
    assert np.median(top) < 0.5 and top.min() > 0.01
    if stochastic:
        assert int((codes != argmin).sum()) > 0
    return dict(codes=codes.numpy().astype(np.int32), logits_pos=flat(logits), soft_pos=flat(soft), loss=per_code.numpy().reshape(B, H, W, D),
                loss_mean=np.float32(loss), loss_depth=depth.numpy())


def main():
    cb, z = SL.codebook(), SL.features()
    q = ref_quantizer(cb)
    out = dict(z=z, temp=np.float32(SL.TEMP), pos=np.array(SL.POS, np.int32), seed=SL.MODEL_SEED, cb_seed=SL.CB_SEED, z_seed=SL.Z_SEED)
    m, _ = mg.ref_rqt(C.RQT_TINY, seed=SL.MODEL_SEED)
    cond = SL.cond(C.RQT_TINY)
    out['cond'] = cond.astype(np.int32)
    for tag, st, seed in (('a_', False, None), ('s_', True, SL.STOCHASTIC_SEED)):
        out.update({tag + k: v for k, v in one_set(m, q, cb, z, cond, st, seed).items()})
    mt, _ = mg.ref_rqt(C.RQT_TINY_TXT, seed=SL.MODEL_SEED)
    cond_t = SL.cond(C.RQT_TINY_TXT)
    out['t_cond'] = cond_t.astype(np.int32)
    out.update({'t_' + k: v for k, v in one_set(mt, q, cb, z, cond_t, False).items()})
    assert np.array_equal(out['t_codes'], out['a_codes'])
    mg.save('rqt_tiny_soft_loss.npz', **out)


if __name__ == '__main__':
    os.chdir(mg.HERE)
    main()
