#!/usr/bin/env python
"""Teacher-forced forward of the ImageNet 1.4B configuration (seeded weights): the stepped path, the one-pass path and log_probs,
device-event times after a warm-up of every shape, the paths alternated in one process.

    python scripts/forward_bench.py [--batches 8,64,500] [--reps 3] [--out profiles/forward_onepass_ab.txt]
    RQ_LIB_PARENT=/path/to/librqamd.so   the stepped path ALSO from a library built from the parent commit (the A/B convention:
                                         each library is its own ctypes handle, one process)
    python scripts/forward_bench.py --trace 64      three one-pass calls in the log_probs form (the same pass; the classifier writes
                                                    sub-chunks that log_prob_kernel reduces) and nothing else: the process to run under
                                                    `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python ...`
    python scripts/forward_bench.py --summarize DIR [--out profiles/forward_onepass_kernel_stats.md]
                                                    kernel shares of that trace (the *kernel_stats.csv below DIR) as a table

Run the process once, under a time limit of its own (timeout -k 10 900 python scripts/forward_bench.py ...)."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'rq-vae-transformer_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

ONE_PASS_KERNELS = ('attn_prefill_kernel', 'attn_packed_kernel', 'log_prob_kernel', 'gather_codes_kernel', 'body_input_kernel',
                    'head_input_kernel', 'resid_ln', 'gemm')


def summarize(directory, out):
    files = sorted(glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True))
    if not files:
        raise SystemExit(f'no *kernel_stats.csv below {directory}')
    rows = list(csv.DictReader(open(files[-1])))
    name_k = 'Name' if 'Name' in rows[0] else 'KernelName'
    tot_k = next(k for k in rows[0] if k.lower().startswith('totalduration'))
    # weight packing (cvt_bf16*, device-to-device parameter copies, bias tables) belongs to loading the model, not to the pass
    rows = [r for r in rows if not any(s in r[name_k] for s in ('cvt_bf16', 'bias_table', 'set_rng', '__amd_rocclr'))]
    total = sum(float(r[tot_k]) for r in rows)
    lines = ['| kernel | calls | total ms | share |', '|---|---:|---:|---:|']
    for r in sorted(rows, key=lambda r: -float(r[tot_k])):
        name = r[name_k].replace('|', '\\|')
        if len(name) > 110:
            name = name[:107] + '...'
        lines.append(f'| `{name}` | {r["Calls"]} | {float(r[tot_k]) / 1e6:.3f} | {100 * float(r[tot_k]) / total:.2f} % |')
    fam = {}
    for r in rows:
        key = next((k for k in ONE_PASS_KERNELS if k in r[name_k]), 'other')
        fam[key] = fam.get(key, 0.0) + float(r[tot_k])
    lines += ['', '| family | total ms | share |', '|---|---:|---:|']
    for k, v in sorted(fam.items(), key=lambda kv: -kv[1]):
        lines.append(f'| {k} | {v / 1e6:.3f} | {100 * v / total:.2f} % |')
    text = '\n'.join(lines) + '\n'
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='8,64,500')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', type=int, default=0)
    ap.add_argument('--summarize', default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.out)

    import numpy as np
    import torch
    import oracle
    from oracle import configs as C
    from rqvae import _native
    from rqvae.models.rqtransformer import RQTransformer

    dev = torch.device('cuda:0')
    cfg = C.RQT_IN_1400M
    V, D = cfg['vocab_size'], cfg['block_size'][2]
    ar = RQTransformer(cfg)
    sd = ar.state_dict()
    with torch.no_grad():
        for k, shp in oracle.rqt_param_shapes(cfg).items():
            sd[k].copy_(torch.from_numpy(oracle.weights.make_tensor(k, shp, 5)))
    ar = ar.to(dev).eval()
    cb = torch.from_numpy(np.random.default_rng(6).standard_normal((V, 256), dtype=np.float32)).to(dev)
    cbs = [cb] * D
    gen = torch.Generator(device='cpu').manual_seed(7)
    stream = torch.cuda.Stream(device=dev)

    def inputs(B):
        return (torch.randint(0, V, (B, 8, 8, D), generator=gen).to(dev), torch.randint(0, cfg['vocab_size_cond'], (B, 1), generator=gen).to(dev))

    eng = ar._eng()                                   # the tree's library
    if a.trace:
        codes, cond = inputs(a.trace)
        with torch.cuda.stream(stream):
            for _ in range(3):
                eng.log_probs(codes, cond, cbs)
        torch.cuda.synchronize()
        return
    paths = {'stepped (tree)': lambda c, k: eng.logits(c, k, cbs), 'one-pass': lambda c, k: eng.forward_onepass(c, k, cbs),
             'log_probs': lambda c, k: eng.log_probs(c, k, cbs)}
    order = ['stepped (tree)', 'one-pass', 'log_probs']
    parent = os.environ.get('RQ_LIB_PARENT')
    if parent:
        mine = _native._lib
        _native._lib = _native._bind(parent, names=[n for n in _native.EXPORTS if n not in ('rqamd_rqt_forward_onepass', 'rqamd_rqt_log_probs')])
        ar._engines = {}
        eng_parent = ar._eng()                        # binds to the parent library for its lifetime
        _native._lib = mine
        paths['stepped (parent library)'] = lambda c, k: eng_parent.logits(c, k, cbs)
        order.insert(0, 'stepped (parent library)')
    lines = [f'# teacher-forced forward, ImageNet 1.4B configuration (seeded weights), device events, median of {a.reps} after warm-up; '
             f'paths alternated in one process' + (f'; parent library: {os.path.basename(os.path.dirname(parent)) or parent}' if parent else '')]
    for B in [int(b) for b in a.batches.split(',')]:
        codes, cond = inputs(B)
        t = {k: [] for k in order}
        with torch.cuda.stream(stream):
            for k in order:                           # warm-up of every shape (workspaces, kernel attributes)
                out = paths[k](codes, cond)
                del out
            for _ in range(a.reps):
                for k in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    out = paths[k](codes, cond)
                    e1.record(stream)
                    e1.synchronize()
                    t[k].append(e0.elapsed_time(e1))
                    del out
        med = {k: float(np.median(v)) for k, v in t.items()}
        base = med.get('stepped (parent library)', med['stepped (tree)'])
        line = f'{B:4d} images: ' + '; '.join(f'{k} {med[k]:8.1f} ms' for k in order) + \
               f'; one-pass {base / med["one-pass"]:.1f}x, log_probs {base / med["log_probs"]:.1f}x the stepped path' + \
               f'; one-pass {B / med["one-pass"] * 1e3:.0f} images/s'
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
