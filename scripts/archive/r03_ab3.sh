#!/bin/bash
# round-3 A/B call 3: halo conv base vs new on one box, barrier timeline, 256x256 GEMM base vs new, short full-batch bench
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
V=rq-vae-transformer_amd/variants
for lib in base new; do
  echo "== conv_halo_bench: $lib"
  if [ $lib = new ]; then unset RQ_LIB; else export RQ_LIB=$PWD/$V/librqamd_$lib.so; fi
  timeout 300 python scripts/conv_halo_bench.py 2>&1 | tail -6
  echo "== gemm_p8_check: $lib"
  RQ_AUTO=1 RQ_MS=10752 timeout 300 python scripts/gemm_p8_check.py 2>&1 | grep -v "^screen" | tail -7
done
unset RQ_LIB
echo "== barrier timeline (new kernel)"
timeout 300 python scripts/conv_trace.py 2>&1 | tail -16 | cut -c1-600
echo "== bench (2 steps, full batch)"
J=$(mktemp)
timeout 600 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --sweep "" 2>&1 | tail -1 > $J
python - $J <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print({k:d.get(k) for k in ('value','ms_per_step','ar_ms_per_image','decode_ms_per_image','verified')})
for k in ('roofline','roofline_decode','roofline_attn'):
    r=d.get(k) or {}
    print(k, r.get('frac'), r.get('avg_launch_us'))
PY
