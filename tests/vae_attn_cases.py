"""Shared by tests/test_gpu_vae_attention.py and tests/test_emu_vae_attention.py: seeded inputs, the fp64 reference and the elementwise
bound of the stand-alone checks of AttnBlock's attention (rqamd_dbg_vae_attn: qkv (B, T, 3C) bf16 -> (B, T, C) bf16).

Reference: fp64 from the bf16-rounded qkv, ref = softmax(q k^T C^-0.5) v, and A = sum_j p_j |v_j|, the magnitude of the same sum.
Bound, elementwise:

    |out - ref| <= 1/2 ulp_bf16(ref) + c 2^-17 A

The first term is the one rounding of the output.  The second is what a kernel may lose before it: the tiled kernel carries the
unnormalised probabilities into its second product as hi + lo of bf16, 16 significant bits, i.e. a relative error of at most 2^-17 per
term (2^-17 A if all of them pointed the same way); the fp32 steps around it (scores over C / 16 MFMA steps, expf, the running rescale,
T / 16 accumulation steps) are each several binary orders below that.  c = 1 would be that analytic worst case; C_BOUND = 0.4 is 3 x the
largest value observed on MI355X (0.1275; tests/test_gpu_vae_attention.py lists them per shape, both test files print them under -s)."""
import numpy as np
import torch

from kernel_check import bf16_ulp

C_BOUND = 0.4
TILE = 64                      # query / key tile of vae_attn_tiled_kernel
FORM_AUTO, FORM_WAVE, FORM_MFMA64, FORM_TILED = 0, 1, 2, 3


def make_qkv(B, T, C, kind, seed):
    """(B, T, 3C) bf16 on the CPU.  'flat': q, k, v ~ N(0, 1), scores ~ N(0, 1).  'peaked': q_i = 8 k_j(i) for one chosen key j(i) per
    query, so that the softmax of most rows is near one-hot (score 8 |k|^2 C^-0.5 ~ 8 sqrt(C) against 8 N(0, 1) elsewhere); j(i) lies
    in the first key tile for queries i = 0 mod 3 (the running max never rises after tile 0), in the last tile for i = 1 mod 3 (it rises
    at the very end) and in a middle tile for the rest (any tile where T has only two)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn((B, T, C), generator=g).bfloat16() for _ in range(3))
    if kind == 'peaked':
        i = torch.arange(T)
        first = torch.randint(0, TILE, (B, T), generator=g)
        last = torch.randint(T - TILE, T, (B, T), generator=g)
        mid = torch.randint(TILE, T - TILE, (B, T), generator=g) if T > 2 * TILE else torch.randint(0, T, (B, T), generator=g)
        win = torch.where(i % 3 == 0, first, torch.where(i % 3 == 1, last, mid))                 # (B, T)
        q = (8.0 * torch.gather(k.float(), 1, win[..., None].expand(B, T, C))).bfloat16()       # exact: a power of two times a bf16 value
    else:
        assert kind == 'flat'
    return torch.cat([q, k, v], dim=-1).contiguous()


def reference(qkv):
    """fp64 (ref, A) of a (B, T, 3C) bf16 qkv, on qkv's device"""
    C = qkv.shape[-1] // 3
    q, k, v = qkv.double().split(C, dim=-1)
    p = torch.softmax(q @ k.transpose(1, 2) * (float(C) ** -0.5), dim=-1)
    return p @ v, p @ v.abs()


def check(out, ref, A, c=C_BOUND, what=''):
    """asserts the elementwise bound; returns (observed max (err - 1/2 ulp) / (2^-17 A), mean |err|)"""
    err = (out.double() - ref).abs()
    half = 0.5 * bf16_ulp(ref)
    unit = 2.0 ** -17 * A
    ratio = float(((err - half).clamp_min(0.0) / unit.clamp_min(1e-300)).max())
    bad = ~(err <= half + c * unit)                       # NaN counts as bad
    if bool(bad.any()):
        t = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} outside the bound (observed c {ratio:.3f} > {c}); first at {t}: '
                             f'out {float(out[t])!r}, ref {float(ref[t])!r}, |err| {float(err[t]):.3e} > {float((half + c * unit)[t]):.3e}')
    return ratio, float(err.mean())


def np_t(a):
    return torch.from_numpy(np.ascontiguousarray(a))
