// rqt_anchor.hip -- anchored sampling: draw codes near an encoded image (gfx950).
//
// An anchored sampling call (rqamd_rqt_sample_anchor in front of a sampling call) adds, at every head step, the quantiser's own soft-code
// term to the logits of image b: x'[v] = x[v] - w(b, p, d) * dist(r_d(b, p), codebook_d[v]), r_0 = z[b, p, :] and r_{d+1} = r_d -
// codebook_d[code(b, p, d)] the residual the image has at that depth given the codes drawn so far.  Three launches per head step, after
// the classifier GEMM and the LogitMask launch and before the sampler:
//   anchor_residual_kernel   r from z and the codes of depths < d at the current position, subtracted in the quantiser's order and bits;
//                            stateless (recomputed from z at every depth), so kept codes need no residual state
//   rq_launch_neg_distances  the quantiser's fp32-MFMA distance kernel (quantize.hip), unchanged, inv_temp = -1: the values of
//                            rqamd_rq_distances over the same rows, bit for bit
//   anchor_fold_kernel       anchor_logit (rqt_kernels.h) over the row -- both twins of a guided pair -- into a scratch; the sampler of
//                            the step reads the scratch like any logits, so every sampler form serves anchored calls with its instruction
//                            stream untouched.  The raw logits stay where they are: the model log-probabilities of an armed call are
//                            defined on them.
// rqamd_anchor_logits is the three stages of one step over given rows, for the host loops and the tests.
//
// The fold is memory-bound, two (guided: three) row reads and one (two) row writes per image and no reuse: 16-byte accesses where every
// row starts on one (V % 4 == 0, aligned bases), 4-byte accesses otherwise (V = 499 of the fixtures).  A workgroup works on ONE row, so
// the weight of the row is a workgroup-uniform load, and the workgroups of a row stride over its columns; the grid is capped near 2048
// workgroups.  Plain stores: the sampler reads the scratch in the next launch (see rqt_compose.hip).
#include "rqt_kernels.h"
#include "rq_common.h"

int rq_launch_neg_distances(const float* x, const float* codebook, const float* code_norms, int n_embed, long n_vec, int dim, float inv_temp,
                            float* logit_out, float* part_v, int* part_i, hipStream_t st);      // quantize.hip

// AnchorResidArgs (rqt_kernels.h): one thread per (row, four dims), the depths one after the other
__global__ __launch_bounds__(256) void anchor_residual_kernel(AnchorResidArgs p) {
    const int f4 = p.dim / 4;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)p.rows * f4) return;
    const long b = gid / f4;
    const int f = (int)(gid - b * f4);
    const long pos = p.pos ? *p.pos : 0;
    f32x4 rv = *(const f32x4*)(p.z + b * p.z_stride + pos * p.dim + f * 4);
    const int64_t* codes = p.codes + b * p.code_stride + pos * p.code_D;
    for (int j = 0; j < p.d; ++j) {
        const long code = codes[j];
        if (code < 0 || code >= p.K) rq_trap();       // an index error in the reference (F.embedding); never a read outside the codebook
        const f32x4 qv = *(const f32x4*)(p.cb[j] + code * p.dim + f * 4);
        rv = rv - qv;
    }
    *(f32x4*)(p.out + b * p.dim + f * 4) = rv;
}

int rq_launch_anchor_resid(const AnchorResidArgs& a, hipStream_t s) {
    if (!a.z || !a.out || a.rows < 0 || a.K < 1) return rq_fail(RQAMD_ERR_INVALID, "anchor_residual: bad argument");
    if (a.d < 0 || a.d > 7 || a.dim < 4 || a.dim % 4) return rq_fail(RQAMD_ERR_INVALID, "anchor_residual: depth %d, dim %d", a.d, a.dim);
    if (a.d > 0 && !a.codes) return rq_fail(RQAMD_ERR_INVALID, "anchor_residual: null codes");
    for (int j = 0; j < a.d; ++j)
        if (!a.cb[j]) return rq_fail(RQAMD_ERR_INVALID, "anchor_residual: null codebook %d", j);
    // 16-byte loads and stores: every row of z, of the codebooks and of the output starts on one (dim % 4 == 0 and aligned bases)
    uintptr_t bases = (uintptr_t)a.z | (uintptr_t)a.out;
    for (int j = 0; j < a.d; ++j) bases |= (uintptr_t)a.cb[j];
    if ((bases & 15) || a.z_stride % 4) return rq_fail(RQAMD_ERR_INVALID, "anchor_residual: z, the codebooks and the output must be 16-byte aligned");
    if (a.rows == 0) return RQAMD_OK;
    const long work = (long)a.rows * (a.dim / 4);
    RQ_LAUNCH(anchor_residual_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, a);
    return rq_check_launch("anchor_residual_kernel");
}

template <bool PAIR>
__global__ __launch_bounds__(256) void anchor_fold_kernel(AnchorFoldArgs p, int chunks, int vec) {
    const int row = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x - (unsigned)row * (unsigned)chunks);
    if (row >= p.rows) return;
    const float w = p.w[(long)row * p.w_row_stride + (long)(p.pos ? *p.pos : 0) * p.D + p.d];
    const long base = (long)row * p.V;
    const float *c = p.c + base, *dist = p.dist + base;
    const float* u = PAIR ? p.u + base : nullptr;
    float* oc = p.out_c + base;
    float* ou = PAIR ? p.out_u + base : nullptr;
    if (vec) {
        const int n4 = p.V >> 2;
        for (int i = chunk * 256 + (int)threadIdx.x; i < n4; i += chunks * 256) {
            const f32x4 cv = *(const f32x4*)(c + 4 * i), dv = *(const f32x4*)(dist + 4 * i);
            f32x4 uv, rc, ru;
            if (PAIR) uv = *(const f32x4*)(u + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                rc[e] = anchor_logit(cv[e], dv[e], w);
                if (PAIR) ru[e] = anchor_logit(uv[e], dv[e], w);
            }
            *(f32x4*)(oc + 4 * i) = rc;
            if (PAIR) *(f32x4*)(ou + 4 * i) = ru;
        }
    } else {
        for (int i = chunk * 256 + (int)threadIdx.x; i < p.V; i += chunks * 256) {
            const float dv = dist[i];
            oc[i] = anchor_logit(c[i], dv, w);
            if (PAIR) ou[i] = anchor_logit(u[i], dv, w);
        }
    }
}

int rq_launch_anchor_fold(const AnchorFoldArgs& a, hipStream_t s) {
    if (!a.c || !a.dist || !a.w || !a.out_c || a.rows < 0 || a.V < 1 || (a.u != nullptr) != (a.out_u != nullptr))
        return rq_fail(RQAMD_ERR_INVALID, "anchor_fold: bad argument");
    if (a.rows == 0) return RQAMD_OK;
    const int vec = a.V % 4 == 0 && (((uintptr_t)a.c | (uintptr_t)a.u | (uintptr_t)a.dist | (uintptr_t)a.out_c | (uintptr_t)a.out_u) & 15) == 0;
    const int per_row = vec ? a.V / 4 : a.V;            // work items of a row
    int chunks = (per_row + 255) / 256;                 // workgroups per row: enough for one pass, at most ~2048 in all
    const int cap = 2048 / a.rows;
    if (chunks > cap) chunks = cap;
    if (chunks < 1) chunks = 1;
    const dim3 grid((unsigned)a.rows * (unsigned)chunks);
    if (a.u) RQ_LAUNCH(anchor_fold_kernel<true>, grid, dim3(256), 0, s, a, chunks, vec);
    else RQ_LAUNCH(anchor_fold_kernel<false>, grid, dim3(256), 0, s, a, chunks, vec);
    return rq_check_launch("anchor_fold_kernel");
}

int rq_launch_anchor_step(const AnchorResidArgs& r, const float* codebook, const float* code_norms, float* dist, float* part_v, int* part_i,
                          const AnchorFoldArgs& f, hipStream_t s) {
    RQ_TRY(rq_launch_anchor_resid(r, s));
    if (r.rows > 0) RQ_TRY(rq_launch_neg_distances(r.out, codebook, code_norms, r.K, (long)r.rows, r.dim, -1.0f, dist, part_v, part_i, s));
    return rq_launch_anchor_fold(f, s);
}

extern "C" int rqamd_anchor_logits(const float* logits, const float* logits_u, const float* z_rows, const int64_t* codes,
                                   const float* const* codebooks, const float* const* code_norms, int d, int dim, int vocab,
                                   const float* weight, int rows, float* out, float* out_u, float* resid_out, float* dist_out,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    if (rows == 0) return RQAMD_OK;
    if (!logits || !z_rows || !codebooks || !code_norms || !weight || !out || !workspace) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: null argument");
    if ((logits_u != nullptr) != (out_u != nullptr)) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: logits_u and out_u go together");
    if (rows < 0 || vocab < 1) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: %d rows, vocab %d", rows, vocab);
    if (d < 0 || d > 7) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: depth %d (0 .. 7)", d);
    if (d > 0 && !codes) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: null codes at depth %d", d);
    if (dim % 64 != 0 || dim < 64 || dim > 256) return rq_fail(RQAMD_ERR_UNSUPPORTED, "anchor_logits: dim %d must be 64, 128, 192 or 256", dim);
    for (int j = 0; j <= d; ++j)
        if (!codebooks[j] || !code_norms[j]) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: null codebook or norms at depth %d", j);
    // workspace: partial minima of the distance kernel (rows * 64 floats and ints), then the residual and the distances where the caller
    // does not ask for them
    const size_t part = (size_t)rows * 64 * 8, rb = resid_out ? 0 : (((size_t)rows * dim * 4 + 255) & ~(size_t)255),
                 db = dist_out ? 0 : (size_t)rows * vocab * 4;
    const size_t need = ((part + 255) & ~(size_t)255) + rb + db;
    if ((size_t)workspace_bytes < need) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: workspace of %zu bytes needed", need);
    if ((uintptr_t)workspace & 15) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: workspace must be 16-byte aligned");
    char* wp = (char*)workspace;
    float* part_v = (float*)wp;
    int* part_i = (int*)(part_v + (size_t)rows * 64);
    wp += (part + 255) & ~(size_t)255;
    float* resid = resid_out ? resid_out : (float*)wp;
    wp += rb;
    float* dist = dist_out ? dist_out : (float*)wp;
    uintptr_t bases = (uintptr_t)resid | (uintptr_t)z_rows;
    for (int j = 0; j <= d; ++j) bases |= (uintptr_t)codebooks[j];
    if (bases & 15) return rq_fail(RQAMD_ERR_INVALID, "anchor_logits: z_rows, resid_out and the codebooks must be 16-byte aligned");
    AnchorResidArgs r{};
    r.z = z_rows; r.z_stride = dim; r.codes = codes; r.code_stride = d; r.code_D = 0; r.pos = nullptr; r.K = vocab; r.d = d; r.dim = dim; r.rows = rows;
    r.out = resid;
    for (int j = 0; j < d; ++j) r.cb[j] = codebooks[j];
    AnchorFoldArgs f{};
    f.c = logits; f.u = logits_u; f.dist = dist; f.w = weight; f.w_row_stride = 1; f.pos = nullptr; f.D = 0; f.d = 0; f.rows = rows; f.V = vocab;
    f.out_c = out; f.out_u = out_u;
    return rq_launch_anchor_step(r, codebooks[d], code_norms[d], dist, part_v, part_i, f, (hipStream_t)stream);
}
