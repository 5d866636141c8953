// rqt_sample_logp.hip -- the LOGP instantiations of the three sampler kernels (the log-probability of every draw: rqamd_sample_logits_logp,
// rqamd_rqt_sample_logp), scalar and per-row, unguided and guided, and their launcher, rq_launch_sample_logp.  The code is the sampler
// section of rqt_kernels.hip, compiled here with LOGP = true; rqt_kernels.hip says why it is an object of its own.
#define RQ_SAMPLE_LOGP_TU 1
#include "rqt_kernels.hip"
