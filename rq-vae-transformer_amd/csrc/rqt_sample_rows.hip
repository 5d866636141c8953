// rqt_sample_rows.hip -- the per-row instantiations of the three sampler kernels (per-image temperature, top-k, top-p, guidance scale
// and Philox seed: rqamd_sample_logits_rows, rqamd_rqt_sample_rows), unguided and guided, and their launcher, rq_launch_sample_per_row.
// The code is the sampler section of rqt_kernels.hip, compiled here with ROWS = true; rqt_kernels.hip says why it is an object of its own.
#define RQ_SAMPLE_ROWS_TU 1
#include "rqt_kernels.hip"
