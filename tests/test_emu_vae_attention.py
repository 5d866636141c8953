"""CPU-only checks of AttnBlock's attention beyond 64 tokens (vae_attn_tiled_kernel, the routing of rq_launch_vae_attn) through the host
emulator (tests/emu): the same .hip sources executed by fibers.  The authoritative runs are the `-m gpu` ones
(tests/test_gpu_vae_attention.py).

1. The kernel alone through rqamd_dbg_vae_attn, forms 1 (wavefront per query) and 3 (tiled), against fp64 with the elementwise bound of
   tests/vae_attn_cases.py.  The emulator's MFMA adds the 16 products of a step in its own order and its expf is the host's, so the
   observed c differs a little from the GPU's (printed); the bound is the same.
2. An RQ-VAE with a 16 x 16 latent (256 tokens at C = 128: five tiled attentions, four key tiles each) end to end against the numpy
   oracle, with the bounds of the tiny model's emulator test (tests/test_emu_kernels.py::test_emu_vae_tiny)."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle
import vae_attn_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import vae_map_cases as V  # noqa: E402

CLANG = os.environ.get('RQ_EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason='no host clang++ for the emulator build')


@pytest.fixture(scope='module')
def nat():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'emu'))
    import build_emu
    path = build_emu.build()
    from rqvae import _native
    import emu_binding
    saved = emu_binding.install(_native, path)
    yield _native
    emu_binding.restore(_native, saved)


@pytest.mark.parametrize('kind', ['flat', 'peaked'])
@pytest.mark.parametrize('shape', [(1, 128, 64), (2, 192, 128)])
def test_emu_vae_attn_forms_vs_fp64(nat, shape, kind):
    """(1, 128, 64): two query tiles x two key tiles, one channel block on two of the four wavefronts.  (2, 192, 128): three tiles, one
    channel block per wavefront, two images.  Form 0 must pick the tiled kernel (bit-identical to form 3)."""
    B, T, C = shape
    qkv = A.make_qkv(B, T, C, kind, seed=7)
    ref, mag = A.reference(qkv)
    outs = {}
    for form in (A.FORM_WAVE, A.FORM_TILED):
        out = torch.full((B, T, C), float('nan'), dtype=torch.bfloat16)
        nat.dbg_vae_attn(qkv, form=form, out=out)
        ratio, mean = A.check(out, ref, mag, what=f'emu form {form} {shape} {kind}')
        print('emu vae attention %s %s form %d: observed c %.4f, mean |err| %.3e' % (shape, kind, form, ratio, mean))
        outs[form] = out
    auto = nat.dbg_vae_attn(qkv, form=A.FORM_AUTO)
    assert torch.equal(auto.view(torch.int16), outs[A.FORM_TILED].view(torch.int16))
    # image 1 of the 2-image launch == its own launch
    if B > 1:
        one = nat.dbg_vae_attn(qkv[1:2].contiguous(), form=A.FORM_TILED)
        assert torch.equal(one.view(torch.int16), outs[A.FORM_TILED][1:2].view(torch.int16))


def test_emu_vae_attn_refusals(nat):
    """what the routing refuses says which limit it hit; a (form, shape) pair the form does not serve is refused as well"""
    def run(T, C, form):
        return nat.dbg_vae_attn(torch.zeros((1, T, 3 * C), dtype=torch.bfloat16), form=form)
    with pytest.raises(NotImplementedError, match='4160 tokens > 4096'):
        run(4160, 64, A.FORM_AUTO)
    with pytest.raises(NotImplementedError, match='1100 tokens > 1024'):
        run(1100, 64, A.FORM_AUTO)
    with pytest.raises(NotImplementedError, match='tiled kernel needs'):
        run(100, 64, A.FORM_TILED)
    with pytest.raises(NotImplementedError, match='tiled kernel needs'):
        run(64, 64, A.FORM_TILED)
    with pytest.raises(NotImplementedError, match='64-token MFMA kernel needs'):
        run(128, 64, A.FORM_MFMA64)
    with pytest.raises(NotImplementedError, match='1088 tokens > 1024'):
        run(1088, 64, A.FORM_WAVE)
    with pytest.raises(ValueError):
        run(128, 64, 4)


def test_emu_vae_latent16_vs_oracle(nat):
    """encode and decode of an RQ-VAE whose mid-block and level-1 AttnBlocks see 256 tokens, against oracle.RQVAEOracle (fp32 numpy)"""
    hps, dd = V.EMU_CFG
    params = oracle.make_params(oracle.rqvae_param_shapes(hps, dd), V.SEED)
    ov = oracle.RQVAEOracle(hps, dd, params)
    eng = nat.VaeEngine(dd, hps['embed_dim'], device='cpu')
    for k, v in params.items():
        if not k.startswith('quantizer.'):
            eng.set_param(k, A.np_t(v))
    x = V.image(V.EMU_CFG)
    z_ref = ov.encode(x)
    z_e = eng.encode(A.np_t(x)).numpy()
    err = np.abs(z_e - z_ref)
    print('emu vae latent 16 x 16 encode: max err %.4f mean %.5f (|ref| max %.3f)' % (err.max(), err.mean(), np.abs(z_ref).max()))
    assert err.max() < 0.05 and err.mean() < 0.008
    codes = ov.get_codes(x)
    cb = params['quantizer.codebooks.0.weight'][:-1]
    dec_ref = ov.decode_code(codes)
    dec = eng.decode(A.np_t(oracle.rq_embed_code(codes, [cb] * 2))).numpy()
    err = np.abs(dec - dec_ref)
    print('emu vae latent 16 x 16 decode: max err %.4f mean %.5f (|ref| max %.3f)' % (err.max(), err.mean(), np.abs(dec_ref).max()))
    assert err.max() < 0.05 and err.mean() < 0.008
