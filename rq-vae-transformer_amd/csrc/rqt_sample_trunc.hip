// rqt_sample_trunc.hip -- the TRUNC instantiations of the sampler kernels (min-p and locally typical sampling after top-p:
// rqamd_sample_logits_trunc, rqamd_rqt_sample_trunc), scalar and per-row, unguided and guided, with or without the log-probability of
// the draw, and their launcher, rq_launch_sample_trunc.  The code is the sampler section of rqt_kernels.hip, compiled here with
// TRUNC = true; rqt_kernels.hip says why it is an object of its own.
#define RQ_SAMPLE_TRUNC_TU 1
#include "rqt_kernels.hip"
