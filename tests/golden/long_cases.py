"""Shared by tests/golden/make_golden_long.py and the long-context tests: the configurations, seeded inputs and stored positions of the
fixtures rqt_long_*.npz (body contexts beyond 256 tokens).  Tiny widths (E 128, two heads of 64, 500 x 64 codebook): a long text prefix
makes a long context without many stepped positions."""
import numpy as np

from oracle import configs as C

CHUNK = 64          # keys per register chunk of attn_long_kernel (8 blocks of 8) and per LDS key tile / query tile of attn_prefill_tiled_kernel


def txt_cfg(block_cond, n_body=1):
    """context 15 + block_cond with only 16 stepped positions"""
    return C.rqt(128, 2, n_body, 1, 500, vocab_cond=20, block_cond=block_cond, block_size=(4, 4, 2), input_embed_dim=64)


def map_cfg():
    """32 x 32 positions behind 64 text tokens: context 1087, the longest the engine accepts but one"""
    return C.rqt(128, 2, 2, 1, 500, vocab_cond=20, block_cond=64, block_size=(32, 32, 2), input_embed_dim=64)


def inputs(cfg, seed, n_img=2):
    """codebook (500, 64), codes (n_img, H, W, D), cond (n_img, block_cond)"""
    rng = np.random.default_rng(seed)
    H, W, D = cfg['block_size']
    cb = rng.standard_normal((cfg['vocab_size'], cfg['input_embed_dim']), dtype=np.float32)
    codes = rng.integers(0, cfg['vocab_size'], (n_img, H, W, D))
    cond = rng.integers(0, cfg['vocab_size_cond'], (n_img, cfg['block_size_cond']))
    return cb, codes, cond


TXT300_SEED, TXT300_INPUT_SEED = 71, 72
MAP_SEED, MAP_INPUT_SEED = 73, 74
# prefix positions of rqt_long_txt300 whose cond_logits are stored (P = 299 prefix tokens: 0 .. 298)
TXT300_COND_POS = [0, 1, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256, 257, 290, 297, 298]


def map_positions():
    """spatial positions (row-major index) of rqt_long_map whose logits are stored: the first two, both sides of every multiple of 256
    body tokens and of the 64-key chunk edges next to them, a block edge and two odd lengths inside a chunk, and the last eight.
    Position pos is body token t = pos + 63 (63 prefix tokens before the first one), which attends over keys 0 .. t."""
    toks = {63, 64}
    for m in (256, 512, 768, 1024):
        for edge in (m - CHUNK, m, m + CHUNK):
            toks.update((edge - 1, edge))
    toks.update((263, 264, 300, 777))
    toks.update(range(1079, 1087))
    return sorted(t - 63 for t in toks if 63 <= t <= 1086)
