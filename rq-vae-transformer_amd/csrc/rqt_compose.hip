// rqt_compose.hip -- composed guidance: the fold of K extra conditionings into the rows of a guided pair (gfx950).
//
// A composed sampling call (rqamd_rqt_sample_compose in front of a guided call) runs (2 + K) B rows up to the classifier: images under
// `cond`, their twins under `uncond`, then K blocks of B rows under the extra conditionings.  Once per head step, after the classifier
// GEMM and the LogitMask launch and before the sampler, compose_kernel<true> reads rows b, B + b and (2 + k) B + b of the raw logits and
// writes c' and u' (rqt_kernels.h: compose_pair) to a scratch of 2 B V floats; the sampler of the step reads the pair from there through
// guide_logit like any guided pair, so every sampler form serves composed calls with its instruction stream untouched.  The raw logits
// stay where they are: the model log-probabilities of an armed call are defined on them.
// compose_kernel<false> is rqamd_compose_logits: guide_logit(c', u', scale) materialised, for the host loops and the tests.
//
// Memory-bound, (K + 2) row reads and 2 row writes (1 for the materialised form) per image and no reuse: 16-byte accesses where every
// row starts on one (V % 4 == 0, aligned bases), 4-byte accesses otherwise (V = 499 of the fixtures).  A workgroup works on ONE row, so
// the K weights of the row are workgroup-uniform loads, and the workgroups of a row stride over its columns; the grid is capped near 2048
// workgroups.  Plain stores: the sampler reads the scratch in the next launch, and non-temporal stores measured negative for outputs
// whose consumer follows directly (profiles/r06_nt_ab.txt).
#include "rqt_kernels.h"
#include "rq_common.h"

static_assert(RQ_MAX_EXTRA_CONDS == RQAMD_RQT_MAX_EXTRA_CONDS, "rqt_kernels.h and include/rqamd.h agree on the number of extra conditions");

template <bool FOLD>
__global__ __launch_bounds__(256) void compose_kernel(ComposeArgs p, int chunks, int vec) {
    const int row = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x - (unsigned)row * (unsigned)chunks);
    if (row >= p.rows) return;
    float w[RQ_MAX_EXTRA_CONDS];
#pragma unroll
    for (int k = 0; k < RQ_MAX_EXTRA_CONDS; ++k) w[k] = k < p.K ? p.w[(long)k * p.rows + row] : 0.f;
    const long base = (long)row * p.V, xstride = (long)p.rows * p.V;
    const float *c = p.c + base, *u = p.u + base, *x = p.x + base;
    float* oc = p.out_c + base;
    float* ou = FOLD ? p.out_u + base : nullptr;
    if (vec) {
        const int n4 = p.V >> 2;
        for (int i = chunk * 256 + (int)threadIdx.x; i < n4; i += chunks * 256) {
            const f32x4 cv = *(const f32x4*)(c + 4 * i), uv = *(const f32x4*)(u + 4 * i);
            f32x4 xv[RQ_MAX_EXTRA_CONDS];
#pragma unroll
            for (int k = 0; k < RQ_MAX_EXTRA_CONDS; ++k)
                if (k < p.K) xv[k] = *(const f32x4*)(x + k * xstride + 4 * i);
            f32x4 rc, ru;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float xe[RQ_MAX_EXTRA_CONDS];
#pragma unroll
                for (int k = 0; k < RQ_MAX_EXTRA_CONDS; ++k) xe[k] = k < p.K ? xv[k][e] : 0.f;
                float c2, u2;
                compose_pair(cv[e], uv[e], xe, w, p.K, c2, u2);
                if (FOLD) { rc[e] = c2; ru[e] = u2; }
                else rc[e] = guide_logit(c2, u2, p.scale);
            }
            *(f32x4*)(oc + 4 * i) = rc;
            if (FOLD) *(f32x4*)(ou + 4 * i) = ru;
        }
    } else {
        for (int i = chunk * 256 + (int)threadIdx.x; i < p.V; i += chunks * 256) {
            float xe[RQ_MAX_EXTRA_CONDS];
#pragma unroll
            for (int k = 0; k < RQ_MAX_EXTRA_CONDS; ++k) xe[k] = k < p.K ? x[k * xstride + i] : 0.f;
            float c2, u2;
            compose_pair(c[i], u[i], xe, w, p.K, c2, u2);
            if (FOLD) { oc[i] = c2; ou[i] = u2; }
            else oc[i] = guide_logit(c2, u2, p.scale);
        }
    }
}

int rq_launch_compose(const ComposeArgs& a, hipStream_t s) {
    if (!a.c || !a.u || !a.x || !a.w || !a.out_c || a.rows < 0 || a.V < 1) return rq_fail(RQAMD_ERR_INVALID, "compose_logits: bad argument");
    if (a.K < 1 || a.K > RQ_MAX_EXTRA_CONDS) return rq_fail(RQAMD_ERR_INVALID, "compose_logits: %d extra conditions (1 .. %d)", a.K, (int)RQ_MAX_EXTRA_CONDS);
    if (!(a.scale - a.scale == 0.f)) return rq_fail(RQAMD_ERR_INVALID, "compose_logits: scale must be finite");
    if (a.rows == 0) return RQAMD_OK;
    const int vec = a.V % 4 == 0 && (((uintptr_t)a.c | (uintptr_t)a.u | (uintptr_t)a.x | (uintptr_t)a.out_c | (uintptr_t)a.out_u) & 15) == 0;
    const int per_row = vec ? a.V / 4 : a.V;            // work items of a row
    int chunks = (per_row + 255) / 256;                 // workgroups per row: enough for one pass, at most ~2048 in all
    const int cap = 2048 / a.rows;
    if (chunks > cap) chunks = cap;
    if (chunks < 1) chunks = 1;
    const dim3 grid((unsigned)a.rows * (unsigned)chunks);
    if (a.out_u) RQ_LAUNCH(compose_kernel<true>, grid, dim3(256), 0, s, a, chunks, vec);
    else RQ_LAUNCH(compose_kernel<false>, grid, dim3(256), 0, s, a, chunks, vec);
    return rq_check_launch("compose_kernel");
}

extern "C" int rqamd_compose_logits(const float* cond_logits, const float* uncond_logits, const float* extra_logits, int n_extra,
                                    const float* extra_weight, int rows, int vocab, float scale, float* out, void* stream) {
    ComposeArgs a{};
    a.c = cond_logits; a.u = uncond_logits; a.x = extra_logits; a.w = extra_weight; a.rows = rows; a.V = vocab; a.K = n_extra;
    a.out_c = out; a.out_u = nullptr; a.scale = scale;
    return rq_launch_compose(a, (hipStream_t)stream);
}
