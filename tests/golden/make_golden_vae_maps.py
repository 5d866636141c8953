#!/usr/bin/env python
"""Generate tests/golden/vae_map{16,32,64}.npz -- RQ-VAEs with 16 x 16, 32 x 32 and 64 x 64 latents whose AttnBlocks see 256, 1024 and
4096 tokens -- by running the REFERENCE ITSELF on the CPU, the way make_golden.py does for vae_tiny.npz (same stub, same seeded weights
through oracle.make_params + load_state_dict(strict=True)).

    python tests/golden/make_golden_vae_maps.py

Needs the reference checkout next to the build (see make_golden.py).  Each fixture stores seeds + the image + reference outputs only; the
configurations live in vae_map_cases.py, which the tests share.  Printed per fixture: numpy oracle vs reference, and the share of codes
whose exact top-2 distance gap exceeds 0.5 (`clear`: the codes a bf16 encoder must reproduce).
"""
import os

import numpy as np

import make_golden as mg          # the reference behind its omegaconf stub, ref_rqvae(), rel(), save()
import vae_map_cases as V
import oracle

torch = mg.torch
MARGIN = 0.5


def gen(name):
    (hps, dd), side, tokens, width = V.CASES[name]
    m, params = mg.ref_rqvae(hps, dd, seed=V.SEED)
    x = V.image((hps, dd))
    with torch.no_grad():
        z_e = m.encode(torch.from_numpy(x))
        out, loss, codes = m(torch.from_numpy(x))
        dec = m.decode_code(codes)
    assert tuple(codes.shape) == (1, side, side, 2)
    ov = oracle.RQVAEOracle(hps, dd, params)
    oz = ov.encode(x)
    cb = params['quantizer.codebooks.0.weight'][:-1]
    gaps, _ = oracle.rq_quantize_margins(z_e.numpy(), [cb] * 2)
    clear = gaps > MARGIN                                  # (1, side, side, 2)
    print(f'  {name}: {tokens} tokens x C {width}; oracle vs ref: encode {np.abs(oz - z_e.numpy()).max():.2e}, '
          f'decode_code {np.abs(ov.decode_code(codes.numpy()) - dec.numpy()).max():.2e}, codes equal {(ov.get_codes(x) == codes.numpy()).mean():.4f}; '
          f'clear codes {clear.mean():.3f}; |z_e| max {np.abs(z_e.numpy()).max():.2f}, |dec| max {np.abs(dec.numpy()).max():.2f}')
    # vae_map64 alone: z_e (64 x 64 x 64) and forward's output stored as fp16, which keeps the file under the repository's 1 MiB limit
    # (|z_e| <= 1.2: the rounding is below 5e-4, a hundredth of the encode bound; decode_code, the same pixels, stays fp32)
    half = np.float16 if name in V.HALF_PRECISION else np.float32
    mg.save(name + '.npz', seed=V.SEED, data_seed=V.DATA_SEED, x=x, z_e=z_e.numpy().astype(half), codes=codes.numpy().astype(np.int32),
            decode_code=dec.numpy(), forward_out=out.numpy().astype(half), loss=np.float32(loss.item()), clear=clear)


if __name__ == '__main__':
    os.chdir(mg.HERE)
    for name in V.CASES:
        gen(name)
