#!/usr/bin/env python
"""Soft-target cross entropy (RQTransformer.soft_target_loss, rqamd_rqt_soft_loss) at the 1.4B shape: E 1536, 24 heads, 42 body + 6 head
layers, 8 x 8 x 4 codes, vocabulary 16384 (oracle.configs.RQT_IN_1400M, random weights), codebook 0.1 N(0,1) and features 0.15 N(0,1) of
dim 256, temp 0.5.  Time per call, device events, one warm-up call per case, the cases alternated in one process, medians and minima of
`reps` runs, B in {8, 64}:

  (a) soft_target_loss(codes, soft_targets=soft)   the soft codes given (their get_soft_codes call is not in the time)
  (b) soft_target_loss(codes, z_e=z, temp=temp)    the soft codes formed inside the engine, per sub-chunk of logits rows
  (h) the host route: forward (one pass) -> (B,8,8,4,16384) fp32 logits, get_soft_codes -> soft codes of the same shape, then the
      reference's formula in torch; with its peak torch.cuda.max_memory_allocated (the engine's own workspace is not torch memory and
      is not in that figure for any of the three)

Losses of the three are compared before anything is timed.  Nothing is asserted about the times.  The output is also written to
profiles/soft_loss_bench.txt.  Optional arguments: the batch sizes (default: 8 64)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'rq-vae-transformer_amd'))
import torch  # noqa: E402
from oracle import configs as cfgs  # noqa: E402
from rqvae import _native  # noqa: E402
from rqvae.models.rqtransformer import RQTransformer  # noqa: E402
from rqvae.models.rqvae.quantizations import RQBottleneck  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device('cuda', 0)
V, DIM, TEMP = 16384, 256, 0.5
OUT = os.path.join(ROOT, 'profiles', 'soft_loss_bench.txt')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


class Aux:
    def __init__(self):
        self.quantizer = RQBottleneck(latent_shape=(8, 8, DIM), code_shape=(8, 8, 4), n_embed=V, shared_codebook=True)
        self.quantizer.codebooks[0].weight[:-1] = 0.1 * torch.randn((V, DIM))
        self.quantizer = self.quantizer.to(dev).eval()


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def time_ms(fns, reps=5):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            res[k].append(timed(f))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in res.items()}


def main(batches):
    say(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'engine_rqt.hip', 'quantize.hip'))}")
    cfg = cfgs.RQT_IN_1400M
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    ar.forward_mode = 'one_pass'
    aux = Aux()
    q = aux.quantizer
    (H, W, D) = cfg['block_size']
    vc = max(cfg['vocab_size_cond'], 1)
    for B in batches:
        z = 0.15 * torch.randn((B, H, W, DIM), device=dev)
        cond = torch.randint(0, vc, (B, 1), device=dev)
        soft, codes = q.get_soft_codes(z, temp=TEMP)

        def form_a():
            return ar.soft_target_loss(codes, aux, cond=cond, soft_targets=soft)

        def form_b():
            return ar.soft_target_loss(codes, aux, cond=cond, z_e=z, temp=TEMP)

        def host():
            logits = ar(codes, aux, cond=cond)
            s, _ = q.get_soft_codes(z, temp=TEMP)
            m = logits.max(-1, keepdim=True)[0]
            logp = logits - m - torch.log(torch.sum(torch.exp(logits - m), -1, keepdim=True) + 1e-7)
            return torch.sum(-s * logp, -1)
        la, lb, lh = form_a(), form_b(), host()
        torch.cuda.synchronize()
        del soft
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        host()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        soft, _ = q.get_soft_codes(z, temp=TEMP)
        out = time_ms({'(a) targets given': form_a, '(b) from features': form_b, '(h) host route': host})
        say(f'== B = {B}, 1.4B shape, {H} x {W} x {D}, V {V}, temp {TEMP}, medians of 5; loss {float(lh.mean()):.4f}; '
            f'max |(a) - (h)| {float((la - lh).abs().max()):.2e}, max |(b) - (h)| {float((lb - lh).abs().max()):.2e}')
        for k, (med, lo) in out.items():
            say(f'  {k:20s} {med:9.2f} ms per call (min {lo:9.2f})')
        say(f'  host route: peak torch memory above the model and the inputs {peak / 2 ** 30:.2f} GiB '
            f'(one (B,H,W,D,V) fp32 tensor is {B * H * W * D * V * 4 / 2 ** 30:.2f} GiB)')
        del soft, la, lb, lh
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as fh:
        fh.write('scripts/soft_loss_bench.py\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [8, 64])
