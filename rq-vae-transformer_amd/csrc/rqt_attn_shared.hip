// rqt_attn_shared.hip -- decode attention of a shared-prompt sampling call (rqamd_rqt_sample_shared): the `fan` rows of a group attend over
// ONE copy of the group's text prefix (keys 0 .. Ps-1, [rows / fan][nh][Ps][64]) and over their own code positions (key j >= Ps is own row
// j - Ps of [rows][nh][Tcap][64]).  Head size 64, bf16 / fp16 caches, contexts of at most 256 keys.
//
// Both forms keep the lane map and the arithmetic order of the kernels they stand next to (csrc/rqt_kernels.hip), so that the output and
// the appended key / value of row r are bit for bit those of attn_decode_kernel / attn_small_kernel on a per-row cache that holds a copy
// of the prefix in front of the row's own positions:
//   register form  attn_run: lane (g, cc) owns 16-byte chunk cc of global key 8 * jj + g, fp32 dot over the chunk then the three DPP steps
//                  of the key group, scores * 1/8, max / sum across the 8 groups by ror8 + four lane reads, exp2 of (s - m) log2(e), fp32
//                  weights on the 16-bit values accumulated block by block, the reduce-scatter over the groups, one rounding.
//   small form     attn_small_run (t <= 7, reached only with Ps < 8): eight (row, head) pairs per wavefront, the per-key pointer
//                  redirected and nothing else.
// What differs is where a key comes from, per lane group: j < Ps from the group's copy, j >= Ps from the row's own cache, so the block
// that straddles Ps mixes the two.  A wavefront serves one (row, head) pair, as in attn_run.  A form in which a wavefront serves 2 or 4
// rows of a group and loads each whole-prefix block once (scores, then the weighted sum, in two passes) was built and measured: it issues
// fewer loads but pays a memory round trip per block, and lost by 40 to 60 % per launch (profiles/shared_cond_bench.txt).  It
// is not in the library.
// The group caches lie in ordinary (cacheable) device memory and the own caches in the uncached KV workspace; the register form reads both
// with the non-temporal loads of attn_run (ld128_nt), the small form reads the group's keys with plain loads.
#include "rqt_kernels.h"
#include "rq_common.h"

static __device__ __forceinline__ void unpack8s(rq_u128 u, float* f) {
    rq_unpack2(u.x, f[0], f[1]);
    rq_unpack2(u.y, f[2], f[3]);
    rq_unpack2(u.z, f[4], f[5]);
    rq_unpack2(u.w, f[6], f[7]);
}
// the score of one key against one query, as attn_run forms it: this lane's 8 components, then the 8 lanes of the key group
static __device__ __forceinline__ float key_dot(const float* qf, rq_u128 kk) {
    float kf[8];
    unpack8s(kk, kf);
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = fmaf(qf[e], kf[e], dot);
    dot += rq_dpp_xor1(dot);
    dot += rq_dpp_xor2(dot);
    dot += rq_dpp_half_mirror(dot);
    return dot;
}

// attn_run with the per-key pointer redirect: one (row, head) pair per wavefront and EVERY global load (q, this token's k | v, all K and V
// blocks) issued before the first use, as there.  NJ = 8-key blocks the launch can hold (blocks >= nblk are skipped at run time).
template <int NJ>
__global__ __launch_bounds__(256) void attn_shared_kernel(AttnSharedArgs p) {
    const int lane = threadIdx.x & 63;
    const int wave = rq_uniform((int)(threadIdx.x >> 6));
    const int hh = blockIdx.x * 4 + wave;
    if (hh >= p.nh) return;
    const int b = (int)blockIdx.y;
    const int t = (p.step ? *p.step : 0) + p.step_off;
    if ((t >> 3) >= NJ || t < p.Ps || t - p.Ps >= p.Tcap) rq_trap();
    const int E = p.E, Ps = p.Ps;
    const int cc = lane & 7, g = lane >> 3;
    const int nblk = (t >> 3) + 1;
    const int tprev = t - 1;
    const float NEG_INF = -__int_as_float(0x7f800000);
    const long spair = (long)(b / p.fan) * p.nh + hh, pair = (long)b * p.nh + hh;
    const bf16_t* ks = p.kcs + spair * Ps * 64;
    const bf16_t* vs = p.vcs + spair * Ps * 64;
    bf16_t* kc = p.kc + pair * p.Tcap * 64;
    bf16_t* vc = p.vc + pair * p.Tcap * 64;
    const bf16_t* qrow = p.qkv + (long)b * 3 * E + hh * 64;
    rq_u128 kr[NJ], vr[NJ];
    const rq_u128 qv = ld128(qrow + cc * 8);
    const rq_u128 kv_new = ld128(qrow + (lane < 8 ? E : 2 * E) + cc * 8);
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        if (jj >= nblk) continue;
        const int j = jj * 8 + g, jc = j < t ? j : tprev;
        kr[jj] = ld128_nt((j >= t ? qrow + E : jc < Ps ? ks + (long)jc * 64 : kc + (long)(jc - Ps) * 64) + cc * 8);
    }
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        if (jj >= nblk) continue;
        const int j = jj * 8 + g, jc = j < t ? j : tprev;
        vr[jj] = ld128_nt((j >= t ? qrow + 2 * E : jc < Ps ? vs + (long)jc * 64 : vc + (long)(jc - Ps) * 64) + cc * 8);
    }
    if (lane < 8) st128(kc + (long)(t - Ps) * 64 + cc * 8, kv_new);
    else if (lane < 16) st128(vc + (long)(t - Ps) * 64 + cc * 8, kv_new);
    float qf[8], sc[NJ];
    unpack8s(qv, qf);
    float mx = NEG_INF;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        float s = NEG_INF;
        if (jj < nblk) {
            const float dot = key_dot(qf, kr[jj]);
            if (jj * 8 + g <= t) s = dot * 0.125f;
        }
        sc[jj] = s;
        mx = fmaxf(mx, s);
    }
    {
        const float m = fmaxf(mx, rq_dpp_ror8(mx));
        mx = fmaxf(fmaxf(rq_readlane(m, 0), rq_readlane(m, 16)), fmaxf(rq_readlane(m, 32), rq_readlane(m, 48)));
    }
    float sum = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        sc[jj] = (sc[jj] == NEG_INF) ? 0.f : rq_fast_exp2((sc[jj] - mx) * 1.4426950408889634f);
        sum += sc[jj];
    }
    sum += rq_dpp_ror8(sum);
    sum = (rq_readlane(sum, 0) + rq_readlane(sum, 16)) + (rq_readlane(sum, 32) + rq_readlane(sum, 48));
    const float inv = 1.0f / sum;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        if (jj >= nblk) continue;
        const float pj = sc[jj] * inv;
        float vf[8];
        unpack8s(vr[jj], vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, vf[e], acc[e]);
    }
    const bool up32 = (lane & 32) != 0, up16 = (lane & 16) != 0, up8 = (lane & 8) != 0;
    float a4[4], a2[2];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float keep = up32 ? acc[e + 4] : acc[e], send = up32 ? acc[e] : acc[e + 4];
        a4[e] = keep + rq_shfl_xor(send, 32);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float keep = up16 ? a4[e + 2] : a4[e], send = up16 ? a4[e] : a4[e + 2];
        a2[e] = keep + rq_shfl_xor(send, 16);
    }
    const float keep1 = up8 ? a2[1] : a2[0], send1 = up8 ? a2[0] : a2[1];
    const float o1 = keep1 + rq_dpp_ror8(send1);
    const int eo = (up32 ? 4 : 0) + (up16 ? 2 : 0) + (up8 ? 1 : 0);
    p.y[(long)b * E + hh * 64 + cc * 8 + eo] = (bf16_t)(pack_bf16x2(o1, 0.f) & 0xffffu);
}

// t <= 7 (Ps < 8): attn_small_run with the per-key pointer redirect -- key j < Ps is the group's, key j >= Ps own row j - Ps
template <int T>
static __device__ __forceinline__ void attn_shared_small_run(const AttnSharedArgs& p, long pair, bool valid, int cc) {
    const int E = p.E, Ps = p.Ps;
    const int b = (int)(pair / p.nh), h = (int)(pair - (long)b * p.nh);
    const bf16_t* qrow = p.qkv + (long)b * 3 * E + h * 64 + cc * 8;
    const long spair = (long)(b / p.fan) * p.nh + h;
    const bf16_t* ks = p.kcs + spair * Ps * 64 + cc * 8;
    const bf16_t* vs = p.vcs + spair * Ps * 64 + cc * 8;
    bf16_t* kc = p.kc + pair * p.Tcap * 64 + cc * 8;
    bf16_t* vc = p.vc + pair * p.Tcap * 64 + cc * 8;
    const rq_u128 qv = ld128(qrow), kn = ld128(qrow + E), vn = ld128(qrow + 2 * E);
    rq_u128 kr[T > 0 ? T : 1], vr[T > 0 ? T : 1];
#pragma unroll
    for (int j = 0; j < T; ++j) kr[j] = j < Ps ? ld128(ks + j * 64) : ld128_nt(kc + (j - Ps) * 64);
#pragma unroll
    for (int j = 0; j < T; ++j) vr[j] = j < Ps ? ld128(vs + j * 64) : ld128_nt(vc + (j - Ps) * 64);
    if (valid) {                                   // append this token's k / v at own row T - Ps
        st128(kc + (T - Ps) * 64, kn);
        st128(vc + (T - Ps) * 64, vn);
    }
    float qf[8], sc[T + 1];
    unpack8s(qv, qf);
    float mx = -__int_as_float(0x7f800000);
#pragma unroll
    for (int j = 0; j <= T; ++j) {
        sc[j] = key_dot(qf, j < T ? kr[j < T ? j : 0] : kn) * 0.125f;
        mx = fmaxf(mx, sc[j]);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j <= T; ++j) {
        sc[j] = rq_fast_exp2((sc[j] - mx) * 1.4426950408889634f);
        sum += sc[j];
    }
    const float inv = 1.0f / sum;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int j = 0; j <= T; ++j) {
        const float pj = sc[j] * inv;
        float vf[8];
        unpack8s(j < T ? vr[j < T ? j : 0] : vn, vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, vf[e], acc[e]);
    }
    if (valid) {
        rq_u128 o;
        o.x = pack_bf16x2(acc[0], acc[1]); o.y = pack_bf16x2(acc[2], acc[3]);
        o.z = pack_bf16x2(acc[4], acc[5]); o.w = pack_bf16x2(acc[6], acc[7]);
        st128(p.y + (long)b * E + h * 64 + cc * 8, o);
    }
}

__global__ __launch_bounds__(256) void attn_shared_small_kernel(AttnSharedArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long total = (long)p.rows * p.nh;
    long pair = ((long)blockIdx.x * 4 + wave) * 8 + (lane >> 3);
    const bool valid = pair < total;
    if (!valid) pair = total - 1;                  // clamped loads, masked stores
    const int t = (p.step ? *p.step : 0) + p.step_off;
    if (t < p.Ps || t - p.Ps >= p.Tcap) rq_trap();
    switch (t) {
        case 1: attn_shared_small_run<1>(p, pair, valid, lane & 7); break;
        case 2: attn_shared_small_run<2>(p, pair, valid, lane & 7); break;
        case 3: attn_shared_small_run<3>(p, pair, valid, lane & 7); break;
        case 4: attn_shared_small_run<4>(p, pair, valid, lane & 7); break;
        case 5: attn_shared_small_run<5>(p, pair, valid, lane & 7); break;
        case 6: attn_shared_small_run<6>(p, pair, valid, lane & 7); break;
        case 7: attn_shared_small_run<7>(p, pair, valid, lane & 7); break;
        default: rq_trap();                        // host bound violated (t >= Ps >= 1)
    }
}

template <int NJ>
static int launch_shared(const AttnSharedArgs& a, hipStream_t s) {
    if (a.rows > 65535) return rq_fail(RQAMD_ERR_UNSUPPORTED, "shared attention: %d rows > 65535", a.rows);
    RQ_LAUNCH((attn_shared_kernel<NJ>), dim3((unsigned)((a.nh + 3) / 4), (unsigned)a.rows), dim3(256), 0, s, a);
    return rq_check_launch("attn_shared_kernel");
}

int rq_launch_attn_shared(const AttnSharedArgs& a, hipStream_t s) {
    if (a.nh < 1 || a.E != a.nh * 64) return rq_fail(RQAMD_ERR_UNSUPPORTED, "shared attention: head size 64 only (E=%d, n_head=%d)", a.E, a.nh);
    if (a.fan < 1 || a.rows < 1 || a.rows % a.fan) return rq_fail(RQAMD_ERR_INVALID, "shared attention: %d rows in groups of %d", a.rows, a.fan);
    if (a.Ps < 1 || a.Tcap < 1 || a.Ps + a.Tcap > 256) return rq_fail(RQAMD_ERR_UNSUPPORTED, "shared attention: prefix %d + %d own positions (1 .. 256 keys)", a.Ps, a.Tcap);
    const int nj_cap = (a.Ps + a.Tcap + 7) / 8;
    int nj = a.t_max >= 0 ? (a.t_max >> 3) + 1 : nj_cap;
    if (nj > nj_cap) nj = nj_cap;
    if (nj == 1) {                                // at most 8 keys: eight pairs per wavefront
        const long pairs = (long)a.rows * a.nh;
        RQ_LAUNCH(attn_shared_small_kernel, dim3((unsigned)((pairs + 31) / 32)), dim3(256), 0, s, a);
        return rq_check_launch("attn_shared_small_kernel");
    }
    if (nj <= 4) return launch_shared<4>(a, s);
    if (nj <= 8) return launch_shared<8>(a, s);
    if (nj <= 16) return launch_shared<16>(a, s);
    return launch_shared<32>(a, s);
}

// diagnostics (include/rqamd.h): the launcher alone, in the style of rqamd_dbg_rqt_attn_decode; what the kernels would trap on is refused here
extern "C" int rqamd_dbg_rqt_attn_shared(const void* qkv, const void* kc_shared, const void* vc_shared, void* kc, void* vc, int rows, int fan,
                                         int nh, int E, int Ps, int Tcap_row, int t, int t_max, int* step_dev, int step_base, void* y,
                                         void* stream) {
    if (!qkv || !y || !kc_shared || !vc_shared || !kc || !vc) return rq_fail(RQAMD_ERR_INVALID, "dbg_rqt_attn_shared: null pointer");
    if (rows < 1 || fan < 1 || rows % fan || nh < 1 || E < 1 || Ps < 1 || Tcap_row < 1)
        return rq_fail(RQAMD_ERR_INVALID, "dbg_rqt_attn_shared: rows %d in groups of %d, n_head %d, embed_dim %d, Ps %d, Tcap_row %d", rows, fan, nh, E, Ps, Tcap_row);
    if (t < Ps) return rq_fail(RQAMD_ERR_INVALID, "dbg_rqt_attn_shared: t %d inside the shared prefix (Ps %d)", t, Ps);
    if (t - Ps >= Tcap_row) return rq_fail(RQAMD_ERR_INVALID, "dbg_rqt_attn_shared: t %d outside the own cache (Ps %d + Tcap_row %d)", t, Ps, Tcap_row);
    if (t_max >= Ps + Tcap_row) return rq_fail(RQAMD_ERR_INVALID, "dbg_rqt_attn_shared: t_max %d outside the caches (%d keys)", t_max, Ps + Tcap_row);
    if (t_max >= 0 && t > t_max) return rq_fail(RQAMD_ERR_INVALID, "dbg_rqt_attn_shared: t %d > t_max %d", t, t_max);
    hipStream_t s = (hipStream_t)stream;
    AttnSharedArgs a;
    a.qkv = (const bf16_t*)qkv; a.kcs = (const bf16_t*)kc_shared; a.vcs = (const bf16_t*)vc_shared; a.kc = (bf16_t*)kc; a.vc = (bf16_t*)vc;
    a.y = (bf16_t*)y; a.step = nullptr; a.step_off = t; a.t_max = t_max;
    a.rows = rows; a.fan = fan; a.nh = nh; a.E = E; a.Ps = Ps; a.Tcap = Tcap_row;
    if (step_dev) {                                   // t = *step_dev + step_off, as the engine's captured graphs pass it
        RQ_TRY(rq_launch_set_int(step_dev, step_base, s));
        a.step = step_dev;
        a.step_off = t - step_base;
    }
    return rq_launch_attn_shared(a, s);
}
