// rqt_sample_sched.hip -- the SCHED instantiations of the per-row sampler kernels (sampling schedules over positions and depths:
// rqamd_rqt_sample_schedule), unguided and guided, plain, with the log-probability of the draw and with the min-p / typical stages, and
// their launcher, rq_launch_sample_sched.  The code is the sampler section of rqt_kernels.hip, compiled here with SCHED = true;
// rqt_kernels.hip says why it is an object of its own.
#define RQ_SAMPLE_SCHED_TU 1
#include "rqt_kernels.hip"
