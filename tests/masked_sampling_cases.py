"""Shared by tests/test_emu_masked_sampling.py (host emulator) and tests/test_gpu_masked_sampling.py (MI355X): models, masks and the
checks of RQTransformer.sample(keep_mask=...).  Every comparison is exact: a masked draw is the unmasked draw of the same (seed, offset,
row, position, depth), and the engine's stepped teacher-forced logits at the same batch go through the kernels the sampling steps use."""
import numpy as np
import torch

import oracle
from oracle import configs as C

SAMPLERS = {'plain': dict(), 'topk_topp': dict(top_k=50, top_p=0.9), 'per_depth': dict(top_k=[50, 40, 30, 20])}
OUT_OF_RANGE = 10 ** 6                    # filler of codes that are not kept: never read, never validated


class Aux:
    """minimal model_aux: only its codebook list is used by the engine"""

    def __init__(self, cb, depth, device):
        t = torch.from_numpy(np.ascontiguousarray(cb)).to(device)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def model(cfg, seed, device):
    """(RQTransformer with seeded weights, model_aux with a seeded codebook -- None for configs without codebook embeddings)"""
    from rqvae.models.rqtransformer import RQTransformer
    ar = RQTransformer(cfg)
    ar.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_params(oracle.rqt_param_shapes(cfg), seed, cfg).items()}, strict=True)
    ar = ar.to(device).eval()
    aux = None
    if ar.config.input_emb_vqvae or ar.config.head_emb_vqvae:
        cb = np.random.default_rng(seed + 1000).standard_normal((max(ar.vocab_size), cfg['input_embed_dim']), dtype=np.float32)
        aux = Aux(cb, cfg['block_size'][2], device)
    return ar, aux


def cond_for(cfg, B, device, seed=5):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, max(cfg['vocab_size_cond'], 1), (B, max(cfg['block_size_cond'], 1)))).to(device)


def seed_all(seed):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def replay_mask(B, H, W, D, seed):
    """Bernoulli(0.5) over (B,H,W,D) from a numpy seed, with the four situations the engine treats differently written in afterwards
    (a fair draw has them with probability ~2 ** -12 per position at B = 3, D = 4):
      p_all   every depth kept in every row          -> an inactive position in the middle: body stack only
      p_row   kept in row 0 only (all depths)        -> the same workgroup grid, one row returns at once
      p_d01   depth 0 drawn, depth 1 kept, all rows  -> a kept depth is conditioned on a drawn one and conditions the next
      last    every depth kept in every row          -> nothing runs after the last active position"""
    keep = np.random.default_rng(seed).random((B, H * W, D)) < 0.5
    p_all, p_row, p_d01, last = (H * W) // 3, (H * W) // 2 + 1, 2, H * W - 1
    assert len({p_all, p_row, p_d01, last}) == 4
    keep[:, p_all] = True
    keep[:, p_row] = False
    keep[0, p_row] = True
    keep[:, p_d01, 0] = False
    if D > 1:
        keep[:, p_d01, 1] = True
    keep[:, last] = True
    act = ~keep.all(axis=(0, 2))
    assert not act[p_all] and not act[last] and act[p_all + 1:].any() and act[:p_all].any()
    return keep.reshape(B, H, W, D)


def check_replay(ar, aux, cond, keep, seed, fillers=(0, OUT_OF_RANGE), **kw):
    """codes0 = the unmasked sample; a masked call that is given codes0 where `keep` is set (and `filler` elsewhere) under the same
    generator state must return codes0, bit for bit"""
    dev = cond.device
    keep_t = torch.from_numpy(keep).to(dev)
    zeros = torch.zeros(keep.shape, dtype=torch.long, device=dev)
    seed_all(seed)
    codes0 = ar.sample(zeros, aux, cond=cond, **kw)
    for filler in fillers:
        partial = torch.where(keep_t, codes0, torch.full_like(codes0, filler))
        given = partial.clone()
        seed_all(seed)
        out = ar.sample(partial, aux, cond=cond, keep_mask=keep_t, **kw)
        assert torch.equal(partial, given)                             # the input is not modified
        assert torch.equal(out[keep_t], codes0[keep_t]), ('kept codes changed', filler, kw)
        assert torch.equal(out, codes0), ('masked draw differs from the unmasked draw', filler, kw)
    return codes0


def kth_largest(logits, k):
    return torch.topk(logits, k, dim=-1).values[..., -1]


def check_support(ar, aux, cond, out, keep_t, partial, top_k, amp=False):
    """every kept code unchanged; the stepped teacher-forced logit of every drawn code is at least the top_k-th largest of its row
    (top_k = 1: it IS the row's maximum)"""
    assert torch.equal(out[keep_t], partial[keep_t])
    logits = ar.teacher_forced_logits(out, aux, cond=cond, amp=amp)
    for d, v in enumerate(ar.vocab_size):                              # LogitMask, as the sampling path applies it
        logits[..., d, v:] = float('-inf')
    drawn = torch.gather(logits, -1, out[..., None])[..., 0]
    ok = drawn >= kth_largest(logits, top_k)
    assert bool(ok[~keep_t].all()), f'{int((~ok & ~keep_t).sum())} drawn codes outside the top-{top_k} support'
