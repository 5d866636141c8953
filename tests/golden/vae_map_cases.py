"""Shared by tests/golden/make_golden_vae_maps.py and the RQ-VAE attention tests: the configurations and seeded inputs of the fixtures
vae_map16 / vae_map32 / vae_map64.npz -- RQ-VAEs whose latent is 16 x 16, 32 x 32 and 64 x 64, with AttnBlocks at the latent resolution
(five each: two in the encoder, three in the decoder) of 256, 1024 and 4096 tokens.  Tiny widths (ch 64, 500 x 64 codebook, depth 2)."""
import numpy as np

from oracle import configs as C

SEED, DATA_SEED = 41, 42          # weights (oracle.make_params) / image


def _cfg(attn_res, ch_mult, resolution):
    return C.vae(n_embed=500, attn_res=(attn_res,), ch=64, ch_mult=ch_mult, resolution=resolution, z_channels=64, embed_dim=64,
                 num_res_blocks=1, depth=2)


# name -> ((hps, ddconfig), latent side, tokens per attention, attention width C)
CASES = {
    'vae_map16': (_cfg(16, (1, 2, 2), 64), 16, 256, 128),
    'vae_map32': (_cfg(32, (1, 2), 64), 32, 1024, 128),
    'vae_map64': (_cfg(64, (1, 1), 128), 64, 4096, 64),
}
HALF_PRECISION = ('vae_map64',)          # fixtures whose z_e / forward_out are stored as fp16 (file size)
# small enough for the host emulator's fibers: 16 x 16 latent out of a 32 x 32 image, 256 tokens at C = 128 (no fixture: the numpy oracle)
EMU_CFG = _cfg(16, (1, 2), 32)


def image(cfg, seed=DATA_SEED, n_img=1):
    """clip(N(0, 1), -1, 1) of the config's resolution, (n_img, 3, R, R) fp32"""
    r = cfg[1]['resolution']
    return np.clip(np.random.default_rng(seed).standard_normal((n_img, 3, r, r), dtype=np.float32), -1, 1)
