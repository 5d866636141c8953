// rqt_sample_guided.hip -- the guided instantiations of the three sampler kernels (classifier-free guidance, rqamd_rqt_sample_guided)
// and their launcher, rq_launch_sample_guided.  The code is the sampler section of rqt_kernels.hip, compiled here with GUIDED = true;
// rqt_kernels.hip says why it is an object of its own.
#define RQ_SAMPLE_GUIDED_TU 1
#include "rqt_kernels.hip"
