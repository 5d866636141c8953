// rqt_attn_extend.hip -- causal multi-token attention that EXTENDS a KV cache which already holds tokens: the attention of the one-pass
// fill of an interior kept run of a masked sampling call ("masked.run_prefill", rqamd_rqt_step_run; engine_rqt.hip: run_prefill).  Per
// (image, head) the cache holds rows 0 .. T0-1; the R new tokens of the run have their q | k | v in qkv [n_img * R][3E].  Query r attends
// over cache rows 0 .. T0-1 and then over the run's own keys 0 .. r (taken from the qkv rows, never from the cache); the k / v of token r
// are appended at cache row T0 + r.  Head size 64, bf16 / fp16 caches, T0 + R <= Tcap <= RQAMD_RQT_MAX_CONTEXT.
//
// The arithmetic is attn_prefill_tiled_kernel's (csrc/rqt_kernels.hip), statement for statement: lane = query, one wavefront per (image,
// head, tile of 64 queries), K / V staged through LDS in tiles of 64 keys -- first the cache rows, then the run's own rows -- and one
// online softmax per query carried across all tiles in key order 0, 1, 2, ...: fp32 dot product in component order, scale 1/8, exp2 of
// (s - m) log2(e), fp32 weights on the 16-bit values, one rounding of the output.  A masked key (an own key beyond the lane's query) gives
// alpha = 1 and w = 0 and leaves m, l and the accumulators as they are, so a query's result does not depend on where the tile edges fall:
// the R outputs and the appended rows are bit for bit those of the prefill kernels over all T0 + R tokens (tests/attn_extend_cases.py).
//
// Lane = query leaves 64 - R lanes idle at small R.  That is accepted: a run replaces R streams of the body weights by one, and the
// attention is a small part of either.  A lane = key mapping would be faster there and would give up the bit-identity.
//
// Reads: cache rows >= T0 are never read (the tests hold NaN there).  Dead lanes clamp to query R-1.  Trip counts are wave-uniform.
// Nothing the launcher accepts reaches a trap -- the kernel has none; every refusal is host-side.
#include "rqt_kernels.h"
#include "rq_common.h"

#define ATTN_EXT_TILE_KEYS 64

static __device__ __forceinline__ void unpack8x(rq_u128 u, float* f) {
    rq_unpack2(u.x, f[0], f[1]);
    rq_unpack2(u.y, f[2], f[3]);
    rq_unpack2(u.z, f[4], f[5]);
    rq_unpack2(u.w, f[6], f[7]);
}

// one staged key against the lane's query: the recurrence of attn_prefill_kernel / attn_prefill_tiled_kernel.  live_key: the key is
// visible to this lane's query (every cached key; an own key j <= iq)
static __device__ __forceinline__ void extend_key(const float (&qf)[64], float (&acc)[64], float& m, float& l, const rq_u128* sK, const rq_u128* sV,
                                                  int jj, bool live_key) {
    const float NEG_INF = -__int_as_float(0x7f800000);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float kf[8];
        unpack8x(sK[jj * 8 + c], kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) dot = fmaf(qf[c * 8 + e], kf[e], dot);
    }
    const float sc = live_key ? dot * 0.125f : NEG_INF;          // 1/sqrt(64), attentions.py:87; causal mask :88-91
    const float mn = fmaxf(m, sc);
    const float alpha = (m == NEG_INF) ? 0.f : rq_fast_exp2((m - mn) * 1.4426950408889634f);
    const float w = (sc == NEG_INF) ? 0.f : rq_fast_exp2((sc - mn) * 1.4426950408889634f);
    l = l * alpha + w;
    m = mn;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float vf[8];
        unpack8x(sV[jj * 8 + c], vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[c * 8 + e] = fmaf(w, vf[e], acc[c * 8 + e] * alpha);
    }
}

__global__ __launch_bounds__(64) void attn_extend_kernel(AttnExtendArgs p) {
    constexpr int KT = ATTN_EXT_TILE_KEYS;
    __shared__ rq_u128 sK[KT * 8], sV[KT * 8];                     // [key][8 chunks of 8 components]
    const int lane = threadIdx.x;
    const int R = p.R, T0 = p.T0, E = p.E;
    const int nqt = (R + 63) / 64;
    const long blk = blockIdx.x;
    const int qt = nqt - 1 - (int)(blk % nqt);                     // the longest tiles of a pair first
    const long pair = blk / nqt;
    const int img = (int)(pair / p.nh), hh = (int)(pair - (long)img * p.nh);
    const bf16_t* q0 = p.qkv + (long)img * R * 3 * E + hh * 64;
    bf16_t* kc = p.kc + pair * p.Tcap * 64;
    bf16_t* vc = p.vc + pair * p.Tcap * 64;
    const int i0 = qt * 64, i = i0 + lane;
    const bool live = i < R;
    const int iq = live ? i : R - 1;
    const float NEG_INF = -__int_as_float(0x7f800000);
    float qf[64], acc[64];
#pragma unroll
    for (int c = 0; c < 8; ++c) unpack8x(ld128(q0 + (long)iq * 3 * E + c * 8), qf + c * 8);
#pragma unroll
    for (int e = 0; e < 64; ++e) acc[e] = 0.f;
    float m = NEG_INF, l = 0.f;
    // ---- the past: cache rows 0 .. T0-1, visible to every query of the run
    for (int j0 = 0; j0 < T0; j0 += KT) {
        const int nk = T0 - j0 < KT ? T0 - j0 : KT;               // keys of this tile (rows >= T0 are not touched)
        rq_syncthreads();                                          // the previous tile has been read
        for (int idx = lane; idx < nk * 8; idx += 64) {
            const long off = (long)(j0 + (idx >> 3)) * 64 + (idx & 7) * 8;
            sK[idx] = ld128(kc + off);
            sV[idx] = ld128(vc + off);
        }
        rq_syncthreads();
        for (int jj = 0; jj < nk; ++jj) extend_key(qf, acc, m, l, sK, sV, jj, true);
    }
    // ---- the run's own keys 0 .. min(i0 + 63, R - 1) from the qkv rows; the diagonal tile is appended at cache rows T0 + j
    const int jend = i0 + 63 < R - 1 ? i0 + 63 : R - 1;           // wave-uniform; lanes mask keys j > i
    for (int j0 = 0; j0 <= jend; j0 += KT) {
        const int nk = jend + 1 - j0 < KT ? jend + 1 - j0 : KT;
        rq_syncthreads();
        for (int idx = lane; idx < nk * 8; idx += 64) {
            const int j = j0 + (idx >> 3), c = idx & 7;
            const rq_u128 kv = ld128(q0 + (long)j * 3 * E + E + c * 8), vv = ld128(q0 + (long)j * 3 * E + 2 * E + c * 8);
            sK[idx] = kv;
            sV[idx] = vv;
            if (j >= i0) {                                         // every row of the run exactly once (T0 + j <= T0 + R - 1 < Tcap)
                st128(kc + (long)(T0 + j) * 64 + c * 8, kv);
                st128(vc + (long)(T0 + j) * 64 + c * 8, vv);
            }
        }
        rq_syncthreads();
        for (int jj = 0; jj < nk; ++jj) extend_key(qf, acc, m, l, sK, sV, jj, j0 + jj <= iq);
    }
    if (live) {
        const float inv = 1.0f / l;
        bf16_t* o = p.y + ((long)img * R + i) * E + hh * 64;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            rq_u128 u;
            u.x = pack_bf16x2(acc[c * 8 + 0] * inv, acc[c * 8 + 1] * inv); u.y = pack_bf16x2(acc[c * 8 + 2] * inv, acc[c * 8 + 3] * inv);
            u.z = pack_bf16x2(acc[c * 8 + 4] * inv, acc[c * 8 + 5] * inv); u.w = pack_bf16x2(acc[c * 8 + 6] * inv, acc[c * 8 + 7] * inv);
            st128(o + c * 8, u);
        }
    }
}

int rq_launch_attn_extend(const AttnExtendArgs& a, hipStream_t s) {
    if (!a.qkv || !a.kc || !a.vc || !a.y) return rq_fail(RQAMD_ERR_INVALID, "extend attention: null pointer");
    if (a.n_img < 1 || a.nh < 1 || a.E < 1 || a.R < 1 || a.T0 < 1)
        return rq_fail(RQAMD_ERR_INVALID, "extend attention: %d images, n_head %d, embed_dim %d, %d new tokens behind %d cached (each >= 1)", a.n_img, a.nh, a.E, a.R, a.T0);
    if (a.Tcap < 1 || a.R > a.Tcap || a.T0 > a.Tcap - a.R)
        return rq_fail(RQAMD_ERR_INVALID, "extend attention: %d cached + %d new tokens (cache %d)", a.T0, a.R, a.Tcap);
    if (a.E / a.nh != 64 || a.E % a.nh) return rq_fail(RQAMD_ERR_UNSUPPORTED, "extend attention: head size 64 only (E=%d, n_head=%d)", a.E, a.nh);
    if (a.Tcap > RQAMD_RQT_MAX_CONTEXT) return rq_fail(RQAMD_ERR_UNSUPPORTED, "extend attention: context %d > RQAMD_RQT_MAX_CONTEXT = %d", a.Tcap, RQAMD_RQT_MAX_CONTEXT);
    const long blocks = (long)a.n_img * a.nh * ((a.R + 63) / 64);
    if (blocks > 0x7fffffffL) return rq_fail(RQAMD_ERR_UNSUPPORTED, "extend attention: %ld (image, head, query tile) triples", blocks);
    RQ_LAUNCH(attn_extend_kernel, dim3((unsigned)blocks), dim3(64), 0, s, a);
    return rq_check_launch("attn_extend_kernel");
}

// diagnostics (include/rqamd.h): the launcher alone, in the style of rqamd_dbg_rqt_attn_prefill; every refusal is the launcher's own
extern "C" int rqamd_dbg_rqt_attn_extend(const void* qkv, void* kc, void* vc, int n_img, int R, int T0, int nh, int E, int Tcap, void* y,
                                         void* stream) {
    AttnExtendArgs a;
    a.qkv = (const bf16_t*)qkv; a.kc = (bf16_t*)kc; a.vc = (bf16_t*)vc; a.y = (bf16_t*)y;
    a.n_img = n_img; a.R = R; a.T0 = T0; a.nh = nh; a.E = E; a.Tcap = Tcap;
    return rq_launch_attn_extend(a, (hipStream_t)stream);
}
