#!/usr/bin/env python
"""Generate tests/golden/rqt_long_*.npz -- body contexts beyond 256 tokens -- by running the REFERENCE ITSELF on the CPU, the way
make_golden.py does for the other fixtures (same stub, same seeded weights through oracle.make_params + load_state_dict(strict=True)).

    python tests/golden/make_golden_long.py

Needs the reference checkout next to the build (see make_golden.py).  Each fixture stores seeds + reference outputs only; the
configurations, inputs and stored positions live in long_cases.py, which the tests share.  Printed for both: numpy oracle vs reference
at these lengths (the emulator tests compare further shapes against the oracle alone).
"""
import os

import numpy as np

import make_golden as mg          # the reference behind its omegaconf stub, ref_rqt(), CodebookAux, save()
import long_cases as L
import oracle

torch = mg.torch


def run(cfg, seed, input_seed):
    m, params = mg.ref_rqt(cfg, seed=seed)
    cb, codes, cond = L.inputs(cfg, input_seed)
    D = cfg['block_size'][2]
    seq, cl = m(torch.from_numpy(codes), mg.CodebookAux(cb), cond=torch.from_numpy(cond))
    seq, cl = seq.numpy(), cl.numpy()
    oseq, ocl = oracle.RQTransformerOracle(cfg, params).forward(codes, [cb] * D, cond, return_cond_logits=True)
    print(f'  oracle vs reference: seq_logits {np.abs(oseq - seq).max():.2e}, cond_logits {np.abs(ocl - cl).max():.2e} '
          f'(|logits| max {np.abs(seq).max():.2f}, context {cfg["block_size"][0] * cfg["block_size"][1] + cfg["block_size_cond"] - 1})')
    return seq, cl, codes, cond


def gen_txt300():
    cfg = L.txt_cfg(300, n_body=2)
    seq, cl, codes, cond = run(cfg, L.TXT300_SEED, L.TXT300_INPUT_SEED)
    mg.save('rqt_long_txt300.npz', seed=L.TXT300_SEED, input_seed=L.TXT300_INPUT_SEED, logits=seq,
            cond_pos=np.array(L.TXT300_COND_POS, np.int32), cond_logits=cl[:, L.TXT300_COND_POS])


def gen_map():
    cfg = L.map_cfg()
    seq, cl, codes, cond = run(cfg, L.MAP_SEED, L.MAP_INPUT_SEED)
    pos = L.map_positions()
    flat = seq.reshape(seq.shape[0], -1, seq.shape[-2], seq.shape[-1])
    cpos = [0, 1, 31, 61, 62]
    mg.save('rqt_long_map.npz', seed=L.MAP_SEED, input_seed=L.MAP_INPUT_SEED, pos=np.array(pos, np.int32), logits=flat[:, pos],
            cond_pos=np.array(cpos, np.int32), cond_logits=cl[:, cpos])


if __name__ == '__main__':
    os.chdir(mg.HERE)
    gen_txt300()
    gen_map()
