#!/usr/bin/env python
"""Log-probabilities of the draws (RQTransformer.return_log_probs(), rqamd_rqt_sample_logp) at the 1.4B shape: E 1536, 24 heads, 42 body +
6 head layers, 8 x 8 x 4 codes, vocabulary 16384 (oracle.configs.RQT_IN_1400M, random weights), captured graphs.  Time per call (the AR
pass), device events, one warm-up call per case (it captures the graphs), armed and unarmed calls alternated in one process, medians and
minima of `reps` runs, B in {64, 500, 2048}:

  (a) unarmed   sample(top_k=1024, top_p=0.95)
  (b) armed     the same call inside return_log_probs(): the LOGP sampler kernels, one log_prob_kernel launch per (position, depth) over
                the B x 16384 fp32 logits rows, two fills ahead of the loop and two (B, 8, 8, 4) fp32 copies after it

(b) is held against (a) of the same run.  An armed step reads the logits rows once more (B x 64 KiB) and adds one small launch:
sample_topk_kernel, which reads the same bytes, is 2.2 % of a headline step, so a few per cent are expected.  The codes of (b) are
compared with those of (a) (same generator state) before anything is timed.  Nothing is asserted about the times.  The output is also
written to profiles/sample_logp_bench.txt.  Optional arguments: the batch sizes (default: 64 500 2048)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'rq-vae-transformer_amd'))
import torch  # noqa: E402
from oracle import configs as cfgs  # noqa: E402
from rqvae import _native  # noqa: E402
from rqvae.models.rqtransformer import RQTransformer  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device('cuda', 0)
TOP_K, TOP_P, V = 1024, 0.95, 16384
OUT = os.path.join(ROOT, 'profiles', 'sample_logp_bench.txt')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


class Aux:
    def __init__(self, V, depth):
        t = torch.randn((V, 256), device=dev)

        class Q:
            @staticmethod
            def codebook_list():
                return [t] * depth
        self.quantizer = Q


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def time_ms(fns, reps=5):
    """fns: name -> callable; one warm-up each, then alternated; returns name -> (median, min) ms per call"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            res[k].append(timed(f))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in res.items()}


def main(batches):
    say(f"{torch.cuda.get_device_name(0)}; kernel sources {_native.kernel_source_hash(('rqt_kernels.hip', 'engine_rqt.hip'))}")
    cfg = cfgs.RQT_IN_1400M
    torch.manual_seed(0)
    with torch.device(dev):
        ar = RQTransformer(cfg).eval()
    aux = Aux(V, 4)
    (H, W, D) = cfg['block_size']
    vc = max(cfg['vocab_size_cond'], 1)
    for B in batches:
        part = torch.zeros((B, H, W, D), dtype=torch.long, device=dev)
        cond = torch.randint(0, vc, (B, 1), device=dev)

        def unarmed():
            return ar.sample(part, aux, cond=cond, top_k=TOP_K, top_p=TOP_P)

        def armed():
            with ar.return_log_probs():
                return ar.sample(part, aux, cond=cond, top_k=TOP_K, top_p=TOP_P)
        torch.cuda.manual_seed_all(B)
        a = unarmed()
        torch.cuda.manual_seed_all(B)
        b, lp = armed()
        same = bool(torch.equal(a, b))
        out = time_ms({'(a) unarmed': unarmed, '(b) armed': armed})
        (ta, tb) = out.values()
        say(f'== B = {B}, 1.4B shape, {H} x {W} x {D}, top_k {TOP_K} / top_p {TOP_P}, graphs, medians of 5; armed codes == unarmed codes: {same}')
        for k, (med, lo) in out.items():
            say(f'  {k:14s} {med:9.2f} ms per call (min {lo:9.2f})')
        say(f'  (b) - (a): {tb[0] - ta[0]:+.2f} ms = {100 * (tb[0] / ta[0] - 1):+.2f} % (medians), {tb[1] - ta[1]:+.2f} ms = '
            f'{100 * (tb[1] / ta[1] - 1):+.2f} % (minima); the extra read of the logits rows is {H * W * D * B * V * 4 / 1e9:.2f} GB per pass')
        say(f'  draw: mean {float(lp.draw.mean()):.4f}; model: mean {float(lp.model.mean()):.4f}, finite {bool(torch.isfinite(lp.model).all())}')
        del a, b, lp
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as fh:
        fh.write('scripts/sample_logp_bench.py\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [64, 500, 2048])
