// engine_rqt.hip -- RQ-Transformer sampling engine (host side of the decode loop, gfx950).
//
// Stands behind RQTransformer.sample / cached_forward (rqvae/models/rqtransformer/transformers.py:190-369),
// AttentionStack.cached_forward / AttentionBlock.cached_forward / MultiSelfAttention.forward
// (attentions.py:60-104,134-142,162-165) and the classifier (transformers.py:90-99,278-285).
//
// Differences from the reference's eager loop, none of which change the math beyond rounding:
//  * only the NEW position is embedded (the reference re-embeds the whole prefix every step,
//    transformers.py:218-225,249-257); sum_d (W e_d + b) is computed as W (sum_d e_d) + D*b,
//  * q/k/v projections are one GEMM over the row-concatenated weight [query;key;value],
//  * the KV cache has fixed capacity and is appended in place (the reference torch.cat's it, :75-76),
//  * residual adds, split-K reduction and LayerNorm are one kernel (resid_ln),
//  * every step-dependent quantity (spatial position, RNG offset) lives in device memory, so the
//    per-position launch sequence (1 body step + D head steps + D sampler calls) is identical for
//    every position and can be captured once as a hipGraph and replayed H*W-1 times; the sampler has
//    no host synchronisation (the reference syncs once per step, rqvae/utils/utils.py:103).
//  * weights are bf16 (fp32 accumulate, fp32 residual stream / LayerNorm / softmax / logits).
//
// Teacher-forced passes (RQTransformer.forward, transformers.py:113-188) exist in two forms: the same stepping over given codes
// (rqamd_rqt_logits / rqamd_rqt_forward: B rows per launch, the kernels sampling uses) and ONE pass over all positions
// (forward_onepass below: rqamd_rqt_forward_onepass / rqamd_rqt_log_probs, no KV cache, a workspace of its own).
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "gemm.h"
#include "rq_common.h"
#include "rqt_kernels.h"

struct RqtLayer {
    bf16_t *wqkv, *wproj, *wfc1, *wfc2;
    float *bqkv, *bproj, *bfc1, *bfc2, *ln1w, *ln1b, *ln2w, *ln2b;
    bf16_t *kc, *vc;   // KV cache (workspace, per batch capacity)
    bf16_t *kcs = nullptr, *vcs = nullptr;   // body layers in the shared-prompt layout (rqamd_rqt_sample_shared): the group caches [groups][nh][P][64]; else null
    float* ksc;        // body layers with the opt-in 8-bit key cache (RQAMD_KV=int8k / int8kv): per-key scales, `kc` then holds bytes; else null
    float* vsc;        // body layers with RQAMD_KV=int8kv: per-value-row scales, `vc` then holds bytes; else null
    int nh;            // attention heads of the layer's stack (body: cfg.n_head; head: the same unless the "head.n_head" option says otherwise)
};

struct GemmProfile {
    bool on = false;
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    double bytes = 0, flops = 0;
    double ms_total = 0;
    int64_t launches = 0;
    // the decode-step attention launches of the same call, bracketed the same way (second roofline: KV-cache bytes / this time)
    std::vector<hipEvent_t> ev_attn;
    size_t used_attn = 0;
    double attn_ms_total = 0;
    int64_t attn_launches = 0;
    // profile == 2: the decode-step GEMM launches are SKIPPED (graphs stay on; everything else runs, on garbage).  The time of a
    // sampling pass minus the time of the same pass without its GEMMs is what the GEMMs cost inside the captured graphs --
    // bracketing every launch with events (profile == 1) runs eagerly and adds the dispatch latency of two markers to a ~7-us kernel.
    bool skip_gemm = false;
};

struct rqamd_rqt {
    rqamd_rqt_config cfg;
    int E, HW, D, V, Din, cond_len, Tbody;
    DevBuf arena;                 // all parameters
    std::vector<RqtLayer> body, head;
    bf16_t *w_in, *w_headin, *w_cls;
    float *b_in, *b_headin, *b_cls, *cls_lnw, *cls_lnb;
    bf16_t* w_ccls = nullptr;                      // cond_classifier (transformers.py:100-104), text-conditioned models only
    float *b_ccls = nullptr, *ccls_lnw = nullptr, *ccls_lnb = nullptr;
    int n_ccls_seen = 0;
    float *cond_emb, *pos_cond, *pos_hw, *pos_d;
    float* tok_emb = nullptr;      // learned token embeddings (variants with input_emb_vqvae / head_emb_vqvae off), fp32 [sum V][E]
    int tok_offs[8] = {}, Vd[8] = {};
    long tok_rows = 0;
    bool in_vq = true, head_vq = true, shared_cls = true, cumsum = true;
    float *body_in_bias, *head_in_bias;   // [HW][E], [D][E] derived tables
    bool tables_dirty = true;
    std::vector<std::string> seen;
    size_t n_required = 0;

    // workspace for `cap` rows
    int cap = 0;
    DevBuf ws, kv;
    float *x, *xh, *slabs, *logits;
    bf16_t *y, *qkv, *ya, *hbuf, *ain;
    int64_t *xs, *cond;
    int* st;            // [0] = spatial position
    uint64_t* rng;      // {seed, offset}
    int* smp_redo;      // [rows] sampler workspace (rows the top-k kernel hands back to the general kernel)
    uint8_t* keep;      // [rows][HW][D] keep flags of a masked sampling call (rqamd_rqt_sample_masked), laid out like xs
    // per-row sampling parameters of rqamd_rqt_sample_rows, filled before the position loop of every such call (outside any capture): the
    // captured per-row graphs hold these addresses, never a value
    float *row_T, *row_gs;      // [rows]
    int* row_tk;                // [rows][D]
    float* row_tp;              // [rows][D]
    uint64_t* row_seed;         // [rows]
    float *row_mp, *row_typ;    // [rows][D] min-p / typical values of a per-row call armed by rqamd_rqt_sample_trunc (both filled, off values where a filter is not given)
    std::vector<char> row_host; // host staging of the arrays: outlives the asynchronous copies of the call that filled it
    // log-probabilities of an armed call (rqamd_rqt_sample_logp), laid out like xs: filled before the position loop (draw 0, model NaN), written
    // by the LOGP samplers and the step form of log_prob_kernel, copied out next to the codes -- the captured graphs hold these addresses
    float *logp_draw, *logp_model;      // [rows][HW][D]
    struct LogpArm { float *draw, *model, *model_u; bool on() const { return draw || model || model_u; } } arm = {};   // outputs of the next sampling call
    // the arming of rqamd_rqt_sample_trunc: HOST arrays, read by the next sampling call (D entries each, or batch * D image-major)
    struct TruncArm { const float *min_p, *typical_p; int per_image; bool on() const { return min_p || typical_p; } } tarm = {};
    // sampling schedules (rqamd_rqt_sample_schedule): the arming -- HOST arrays of HW * D values (per_image: batch * HW * D, image-major),
    // read by the next sampling call -- and the device tables the scheduled sampler launches read at [row * row_stride + pos * D + d].
    // `sch_shared` ([HW][D] each, row_stride 0) comes from the slab; `sch_image` ([images][HW][D] each) is memory of its own, allocated by
    // the first call that needs it, outside any capture, and kept -- it grows with the batch, which drops the graphs that hold its addresses.
    // Every table a call's launches read is filled before the position loop, the captured graphs hold addresses only
    struct SchedArm {
        const float* temperature; const int* top_k; const float *top_p, *gscale, *min_p, *typical_p; int per_image;
        bool on() const { return temperature || top_k || top_p || gscale || min_p || typical_p; }
    } sarm = {};
    struct SchedTables { float* T; int* tk; float *tp, *gs, *mp, *typ; } sch_shared = {}, sch_image = {};
    DevBuf sch_image_buf;
    size_t sch_image_rows = 0;      // images the tables of sch_image hold
    std::vector<char> sch_host;     // host staging of the tables, like row_host
    // shared-prompt sampling (rqamd_rqt_sample_shared): the arming, and the layout of the KV workspace.  kv_groups == 0: the plain layout
    // (body caches of Tbody slots per (row, head) in h->kv).  kv_groups > 0: the shared layout -- body caches of HW own slots per (row, head)
    // in h->kv, and group caches of P = cond_len - 1 slots per (group, head) for up to kv_groups groups in h->kvg.  h->kvg is ordinary cached
    // memory: every line of it is read `fan` times per position and again at the next one, where h->kv is written once and read once per
    // position (uncached).  One layout at a time: a call in the other form re-lays the workspace (ensure_batch), which drops every graph.
    int shared_fan = 0;
    int cur_fan = 0;       // rows per group of the shared-prompt call being run (the body stack's attention launches read it)
    int kv_groups = 0;
    DevBuf kvg;
    // composed guidance (rqamd_rqt_sample_compose): the arming -- the extra conditionings (device pointers, copied when the call arms) and
    // the HOST weights (n * batch, read by the next sampling call) -- and what the fold launches of such a call use: a scratch of 2 B V
    // floats (c', u': rqt_compose.hip) and the device weight table (K, B), memory of their own, allocated by the first composed call
    // outside any capture and kept; they grow with the batch, which drops the composed graphs that hold their addresses
    struct ComposeArm { int n; const int64_t* cond[RQ_MAX_EXTRA_CONDS]; const float* weight; } carm = {};
    DevBuf cmp_buf;
    float *cmp_logits = nullptr, *cmp_w = nullptr;
    size_t cmp_rows = 0;            // images the two hold
    std::vector<float> cmp_host;    // host staging of the weight table, like row_host
    // anchored sampling (rqamd_rqt_sample_anchor): the arming -- z and the codebooks / norms (device pointers, the two pointer ARRAYS copied
    // when the call arms) and the HOST weights (HW * D, per_image: batch * HW * D, read by the next sampling call) -- and what the three
    // launches per head step of such a call use (rqt_anchor.hip), one block of memory of the handle's own, allocated by the first
    // anchored call outside any capture and kept: the logits scratch (rows * V floats, rows = the images, twice that for guided calls),
    // the distances (images * V), the residual (images * dim), the partial minima of the distance kernel (images * 64 * 8 bytes), the copy
    // of z (images * HW * dim) and the weight table (images * HW * D; a shared table is repeated for every image, so the captured fold
    // launches hold one row stride).  It grows with the batch or the width of z, which drops the anchored graphs that hold its addresses
    struct AnchorArm { const float* z; const float* cb[8]; const float* cn[8]; int dim; const float* weight; int per_image; int bad; } aarm = {};
    DevBuf anc_buf;
    float *anc_logits = nullptr, *anc_dist = nullptr, *anc_resid = nullptr, *anc_pv = nullptr, *anc_z = nullptr, *anc_w = nullptr;
    int* anc_pi = nullptr;
    size_t anc_imgs = 0, anc_lrows = 0, anc_dim = 0;      // images, logits rows and width of z the block holds
    std::vector<float> anc_host;    // host staging of the weight table, like row_host
    int max_slabs = 8;
    int cur_gelu_v2 = 0;   // GELU form of the stack being run (cfg.gelu_v2: 0 both erf, 1 both sigmoid, 2 body erf / head sigmoid, 3 body sigmoid / head erf)
    bool kv_int8k = false;   // RQAMD_KV=int8k / int8kv when the handle was created: body-stack keys cached as 64 bytes + one fp32 scale (rqt_kernels.hip)
    bool kv_int8v = false;   // RQAMD_KV=int8kv: the body-stack values likewise (round 6)

    // graph cache
    // one captured position per 8-key bucket of the body context (the attention kernel variant is baked in); the last one is the catch-all of
    // contexts beyond 256 tokens: captured once with t_max = Tbody - 1, it serves every position from token 256 on (position_body)
    // four sets: [0] unmasked sampling, [1] masked sampling (the sampler launches carry the keep-flag pointer, a kernel argument),
    // [2] / [3] the same two forms of guided sampling (rqamd_rqt_sample_guided: 2B rows, other sampler kernels).  The two sets of a
    // family are captured under the same key, so a caller that alternates between the forms replays what it captured before.  The
    // families have a key each (gkey[0] unguided, gkey[1] guided: B is the 2B rows of the engine and the guidance scale is part of
    // it): a key change drops the two sets of its own family only (gstale), gvalid = false drops all of them.
    // [4] .. [7]: the same four forms of per-row calls (rqamd_rqt_sample_rows), families gkey[2] unguided and gkey[3] guided, and
    // [8] .. [11] (gkey[4], gkey[5]) those of per-row calls with per-image seeds: whether the sampler reads h->row_seed or h->rng is a
    // kernel argument of the captured launch, so seeded calls must never replay unseeded graphs, and neither recaptures the other's.  Their
    // sampler launches read every parameter from h->row_*, so their keys hold no parameter value (T, gs, tk, tp stay zero): rows,
    // codebooks, stream and the guided flag only, and a call with other values replays what is there.  Scalar and per-row families
    // never invalidate each other.  Armed calls (rqamd_rqt_sample_logp: other sampler kernels and one more launch per step) are six
    // more families, gkey[6] .. gkey[11] and sets [12] .. [23], in the same order: alternating armed and unarmed calls recaptures nothing.
    // Calls with min-p / typical sampling in effect (rqamd_rqt_sample_trunc: other sampler kernels at the depths with a filter on) are
    // all twelve once more, gkey[12] .. gkey[23] and sets [24] .. [47].  Their scalar values are in the key next to tk / tp (mp, typ:
    // zero in every other family's key); per-image values are in h->row_mp / h->row_typ and in no key.
    // Scheduled calls (rqamd_rqt_sample_schedule: the scheduled per-row sampler kernels) are 32 more families, gkey[24] .. gkey[55] and
    // sets [48] .. [111] (step_family: filters / armed / seeded / per-image tables / guided, a bit each).  Every value is in a table, so
    // like the per-row keys theirs hold rows, codebooks, stream and the guided flag alone: other values replay the same graphs, and
    // scalar, per-row and scheduled families never invalidate each other.
    static constexpr int NGRAPH = 33;
    static constexpr int NFAM_SCHED0 = 24;         // first scheduled family
    static constexpr int NFAM = 56;
    // Shared-prompt calls (rqamd_rqt_sample_shared: another attention launch in the body stack, other cache addresses) are every family
    // once more, keys NFAM .. 2 * NFAM - 1 and sets 2 * NFAM .. 4 * NFAM - 1 (graph_family); the group size is part of their key.
    // Composed calls (rqamd_rqt_sample_compose: (2 + K) B rows, a fold launch per head step, the sampler reads the scratch) are every family
    // a third time, keys 2 * NFAM .. 3 * NFAM - 1 and sets 4 * NFAM .. 6 * NFAM - 1; K is part of their key next to the rows, no weight is.
    // Anchored calls (rqamd_rqt_sample_anchor: three more launches per head step, the sampler reads the scratch) are every family a fourth
    // time, keys 3 * NFAM .. 4 * NFAM - 1 and sets 6 * NFAM .. 8 * NFAM - 1.  Next to the fields of the family the call would otherwise
    // belong to, their key holds the codebook and norms pointers of the arming and the width of z (kernel arguments of the captured
    // launches, as `cb` is); z and the weights live in memory of the handle and are in no key.
    hipGraphExec_t gexec[8 * NFAM][NGRAPH] = {};
    struct Key {
        int B; float T; float gs; int guided; int tk[8]; float tp[8]; const float* cb[8]; void* stream; float mp[8]; float typ[8]; int fan; int n_extra;
        const float* acb[8]; const float* acn[8]; long adim;
    } gkey[4 * NFAM];
    bool gkey_set[4 * NFAM] = {}, gstale[4 * NFAM] = {};
    bool gvalid = false;
    int64_t n_capture = 0;     // position graphs captured over the life of the handle (rqamd_rqt_graph_captures)

    GemmProfile prof;

    // stepping form (rqamd_rqt_step_*): one (position, depth) step per call, the caller draws the samples
    bool step_on = false;
    int step_B = 0, step_pos = 0, step_d = 0;      // next expected step
    const float* step_cb[8] = {};
    const float* step_pend_slabs = nullptr;        // the body's last fc2 partials, consumed by depth 0 of the same position
    int step_pend_n = 0;
    const float* step_pend_bias = nullptr;

    // one-pass teacher-forced forward (forward_onepass): a workspace of its own, sized by a row budget per chunk -- never h->ws / h->kv,
    // whose addresses the captured sampling graphs hold
    int fwd_chunk_rows = 4096;    // "fwd.chunk_rows": body rows per chunk of images, head rows per sub-chunk
    int fwd_logits_bytes = 48 << 20;   // "fwd.logits_bytes": the logits sub-chunk the log_probs / soft_loss forms reduce (whole depth groups, at least one)
    DevBuf fws;
    // "prefix.one_pass": the given leading positions of a sampling call fill the KV cache in one pass (prefix_prefill) instead of one
    // body-only step each.  Off by default; the captured graphs are the same either way, so the option invalidates nothing
    bool prefix_one_pass = false;
    // "masked.run_prefill": every kept run of a sampling call that is not leading -- two or more consecutive positions at which no head
    // runs, behind position 0 and behind whatever "prefix.one_pass" covered, with a drawn position after it -- fills its KV rows in one pass
    // (run_prefill) instead of one body-only step per position.  Off by default; the position graphs are the same either way
    bool masked_run_prefill = false;
};

// -------------------------------------------------------------------------------------------------
__global__ void bias_table_kernel(const float* bias, float scale, const float* pos, float* out, int rows, int E) {
    long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)rows * E) return;
    int e = (int)(gid % E);
    out[gid] = scale * bias[e] + pos[gid];
}
__global__ void set_rng_kernel(uint64_t* rng, uint64_t seed, uint64_t offset) {
    if (threadIdx.x == 0) { rng[0] = seed; rng[1] = offset; }
}
// dst row r = src row r / fan (rows of `len` words): the conditioning of a shared-prompt call, one row per group, for every row of the batch
__global__ void repeat_rows_kernel(const int64_t* src, int64_t* dst, long rows, int len, int fan) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= rows * len) return;
    const long r = gid / len;
    dst[gid] = src[(r / fan) * len + (gid - r * len)];
}
__global__ void fill_f32_kernel(float* p, float v, long n) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < n) p[gid] = v;
}

static size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" int rqamd_rqt_create(const rqamd_rqt_config* c, rqamd_rqt** out) {
    if (!c || !out) return rq_fail(RQAMD_ERR_INVALID, "rqt_create: null argument");
    if (c->n_head < 1 || c->embed_dim % c->n_head || c->embed_dim / c->n_head > 256)      // 64 is what the tuned kernels take; any other size <= 256: the plain attention kernel
        return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_create: embed_dim=%d must be a multiple of n_head=%d with head_dim <= 256", c->embed_dim, c->n_head);
    if (c->embed_dim % 64 || c->input_embed_dim % 64 || c->embed_dim > 4096)
        return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_create: embed_dim / input_embed_dim must be multiples of 64, embed_dim <= 4096");
    if (c->n_layer_body < 1 || c->n_layer_head < 0)      // head.n_layer = 0: the depth-1 "VQ-GAN" shapes (measure_throughput/__main__.py:166-210)
        return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_create: needs >= 1 body layer and >= 0 head layers");
    if (c->D < 1 || c->D > 8 || c->H < 1 || c->W < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_create: bad block_size");
    if (c->gelu_v2 < 0 || c->gelu_v2 > 3) return rq_fail(RQAMD_ERR_INVALID, "rqt_create: gelu_v2 = %d (0 .. 3)", c->gelu_v2);
    rqamd_rqt* h = new rqamd_rqt();
    h->cfg = *c;
    {   // opt-in storage format of the body stack's key cache, fixed for the life of the handle (default: bf16, what BASELINE.json asks for)
        const char* kvf = getenv("RQAMD_KV");
        if (kvf && *kvf && strcmp(kvf, "bf16") != 0) {
            if (strcmp(kvf, "int8k") != 0 && strcmp(kvf, "int8kv") != 0) { delete h; return rq_fail(RQAMD_ERR_INVALID, "rqt_create: RQAMD_KV=%s (bf16, int8k or int8kv)", kvf); }
            if (c->embed_dim != c->n_head * 64) { delete h; return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_create: RQAMD_KV=%s is written for head_dim 64 (embed_dim=%d n_head=%d)", kvf, c->embed_dim, c->n_head); }
            h->kv_int8k = true;
            h->kv_int8v = strcmp(kvf, "int8kv") == 0;
        }
    }
    h->E = c->embed_dim; h->HW = c->H * c->W; h->D = c->D; h->V = c->vocab_size; h->Din = c->input_embed_dim;
    h->cond_len = c->block_size_cond < 1 ? 1 : c->block_size_cond;
    h->Tbody = h->HW + h->cond_len - 1;
    if (h->Tbody > RQAMD_RQT_MAX_CONTEXT) {
        const int tb = h->Tbody;
        delete h;
        return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_create: context %d > RQAMD_RQT_MAX_CONTEXT = %d", tb, RQAMD_RQT_MAX_CONTEXT);
    }
    if (h->Tbody > 256) {      // the chunked decode attention and the tiled prefill: head size 64, bf16 / fp16 cache (rqt_kernels.hip)
        const int tb = h->Tbody;
        if (h->kv_int8k) { delete h; return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_create: context %d > 256 with RQAMD_KV=%s (the 8-bit cache formats end at 256 tokens)", tb, getenv("RQAMD_KV")); }
        if (c->embed_dim != c->n_head * 64) {
            delete h;
            return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_create: context %d > 256 needs head size 64 in the body stack (embed_dim=%d n_head=%d)", tb, c->embed_dim, c->n_head);
        }
    }
    const size_t E = h->E, V = h->V, Din = h->Din;
    const int vc = c->vocab_size_cond < 1 ? 1 : c->vocab_size_cond;
    const size_t per_layer = al(3 * E * E * 2) + al(E * E * 2) + 2 * al(4 * E * E * 2) + al(3 * E * 4) + al(4 * E * 4) + 6 * al(E * 4);
    size_t total = per_layer * (c->n_layer_body + c->n_layer_head) + 2 * al(E * Din * 2) + al(V * E * 2) + 4 * al(E * 4) + al(V * 4)
                   + al(vc * E * 4) + al(h->cond_len * E * 4) + 2 * al(h->HW * E * 4) + 2 * al(h->D * E * 4);
    if (h->cond_len > 1) total += al((size_t)vc * E * 2) + al((size_t)vc * 4) + 2 * al(E * 4);
    // stage-2 flag variants (a struct zero-filled by an old caller means "all on", i.e. the released configuration)
    const bool legacy = c->vocab_sizes[0] == 0;
    h->in_vq = legacy || c->input_emb_vqvae; h->head_vq = legacy || c->head_emb_vqvae;
    h->shared_cls = legacy || c->shared_cls_emb; h->cumsum = legacy || c->cumsum_depth_ctx;
    for (int d = 0; d < c->D; ++d) {
        h->Vd[d] = legacy ? c->vocab_size : c->vocab_sizes[d];
        if (h->Vd[d] < 1 || h->Vd[d] > c->vocab_size) { delete h; return rq_fail(RQAMD_ERR_INVALID, "rqt_create: vocab_sizes[%d] = %d not in 1..vocab_size", d, h->Vd[d]); }
    }
    if (!(h->in_vq && h->head_vq)) {
        const bool shared_tok = legacy || c->shared_tok_emb;
        // one shared table has Vd[0] rows: a depth with a larger vocabulary would read past it (the reference asserts equal
        // vocabularies for shared_tok_emb, transformers.py:55-56, and nn.Embedding raises an index error)
        for (int d = 0; shared_tok && d < c->D; ++d)
            if (h->Vd[d] > h->Vd[0]) {
                const int vd = h->Vd[d], v0 = h->Vd[0];
                delete h;
                return rq_fail(RQAMD_ERR_INVALID, "rqt_create: shared_tok_emb with vocab_sizes[%d] = %d > vocab_sizes[0] = %d", d, vd, v0);
            }
        long rows = 0;
        for (int d = 0; d < c->D; ++d) { h->tok_offs[d] = shared_tok ? 0 : (int)rows; rows += h->Vd[d]; }
        h->tok_rows = shared_tok ? h->Vd[0] : rows;
        total += al((size_t)h->tok_rows * E * 4);
    }
    if (!h->shared_cls) total += al((size_t)c->D * V * E * 2) + al((size_t)c->D * V * 4);
    { const int rc = h->arena.reserve(total); if (rc != RQAMD_OK) { delete h; return rc; } }
    char* p = (char*)h->arena.p;
    auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return (void*)r; };
    auto mk = [&](std::vector<RqtLayer>& v, int n) {
        v.resize(n);
        for (auto& L : v) {
            L.wqkv = (bf16_t*)take(3 * E * E * 2); L.wproj = (bf16_t*)take(E * E * 2);
            L.wfc1 = (bf16_t*)take(4 * E * E * 2); L.wfc2 = (bf16_t*)take(4 * E * E * 2);
            L.bqkv = (float*)take(3 * E * 4); L.bfc1 = (float*)take(4 * E * 4);
            L.bproj = (float*)take(E * 4); L.bfc2 = (float*)take(E * 4);
            L.ln1w = (float*)take(E * 4); L.ln1b = (float*)take(E * 4); L.ln2w = (float*)take(E * 4); L.ln2b = (float*)take(E * 4);
            L.kc = L.vc = nullptr;
            L.ksc = L.vsc = nullptr;
            L.nh = c->n_head;
        }
    };
    mk(h->body, c->n_layer_body);
    mk(h->head, c->n_layer_head);
    h->w_in = (bf16_t*)take(E * Din * 2); h->w_headin = (bf16_t*)take(E * Din * 2);
    h->w_cls = (bf16_t*)take((h->shared_cls ? 1 : (size_t)c->D) * V * E * 2);
    h->b_in = (float*)take(E * 4); h->b_headin = (float*)take(E * 4); h->cls_lnw = (float*)take(E * 4); h->cls_lnb = (float*)take(E * 4);
    h->b_cls = (float*)take((h->shared_cls ? 1 : (size_t)c->D) * V * 4);
    if (h->tok_rows) h->tok_emb = (float*)take((size_t)h->tok_rows * E * 4);
    h->cond_emb = (float*)take(vc * E * 4); h->pos_cond = (float*)take(h->cond_len * E * 4);
    h->pos_hw = (float*)take(h->HW * E * 4); h->body_in_bias = (float*)take(h->HW * E * 4);
    h->pos_d = (float*)take(h->D * E * 4); h->head_in_bias = (float*)take(h->D * E * 4);
    if (h->cond_len > 1) {
        h->w_ccls = (bf16_t*)take((size_t)vc * E * 2); h->b_ccls = (float*)take((size_t)vc * 4);
        h->ccls_lnw = (float*)take(E * 4); h->ccls_lnb = (float*)take(E * 4);
    }
    h->n_required = 4 + 4 + 4 + 12 * 2 * 0;   // filled below
    h->n_required = 3 /*pos*/ + 1 /*cond_emb*/ + (h->in_vq ? 2 : 0) + (h->head_vq ? 2 : 0) + (h->tok_rows ? 1 : 0) + 4 /*classifier*/
                    + (size_t)16 * (c->n_layer_body + c->n_layer_head);
    *out = h;
    return RQAMD_OK;
}

extern "C" int rqamd_rqt_destroy(rqamd_rqt* h) {
    if (!h) return RQAMD_OK;
    for (auto& set : h->gexec) for (auto& g : set) if (g) (void)hipGraphExecDestroy(g);
    for (auto e : h->prof.ev) (void)hipEventDestroy(e);
    for (auto e : h->prof.ev_attn) (void)hipEventDestroy(e);
    delete h;
    return RQAMD_OK;
}

// options of a handle that the config struct does not carry (include/rqamd.h)
extern "C" int rqamd_rqt_set_option(rqamd_rqt* h, const char* name, int value) {
    if (!h || !name) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_option: null argument");
    if (strcmp(name, "head.n_head") == 0) {      // head.block.n_head where it differs from body.block.n_head (transformers.py:86-87: the stacks have their own block configs)
        if (value < 1 || h->E % value || h->E / value > 256)
            return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_set_option: embed_dim=%d must be a multiple of head.n_head=%d with head_dim <= 256", h->E, value);
        for (auto& L : h->head) L.nh = value;
        h->gvalid = false;                       // captured graphs hold the old launches
        return RQAMD_OK;
    }
    if (strcmp(name, "fwd.chunk_rows") == 0) {   // row budget of the one-pass forward's chunks (tests force several chunks on a tiny model)
        if (value < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_option: fwd.chunk_rows = %d < 1", value);
        h->fwd_chunk_rows = value;
        return RQAMD_OK;
    }
    if (strcmp(name, "fwd.logits_bytes") == 0) { // size of the logits sub-chunk of rqamd_rqt_log_probs / rqamd_rqt_soft_loss (tests force the classifier loop to split)
        if (value < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_option: fwd.logits_bytes = %d < 1", value);
        h->fwd_logits_bytes = value;
        return RQAMD_OK;
    }
    if (strcmp(name, "prefix.one_pass") == 0) {  // how the sampling entry points fill the KV cache for the given leading positions (include/rqamd.h)
        if (value != 0 && value != 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_option: prefix.one_pass = %d (0 or 1)", value);
        h->prefix_one_pass = value == 1;
        return RQAMD_OK;
    }
    if (strcmp(name, "masked.run_prefill") == 0) {  // how the sampling entry points fill the KV cache for kept runs that are not leading (include/rqamd.h)
        if (value != 0 && value != 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_option: masked.run_prefill = %d (0 or 1)", value);
        h->masked_run_prefill = value == 1;
        return RQAMD_OK;
    }
    return rq_fail(RQAMD_ERR_INVALID, "rqt_set_option: unknown option '%s'", name);
}

static long numel(const int64_t* shape, int ndim) {
    long n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    return n;
}

extern "C" int rqamd_rqt_set_param(rqamd_rqt* h, const char* name, const float* src, const int64_t* shape, int ndim, void* stream) {
    if (!h || !name || !src || !shape) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_param: null argument");
    hipStream_t st = (hipStream_t)stream;
    const long n = numel(shape, ndim);
    const long E = h->E;
    std::string s(name);
    auto expect = [&](long want) -> int {
        if (n != want) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_param(%s): %ld elements, expected %ld", name, n, want);
        return RQAMD_OK;
    };
    auto f32copy = [&](float* dst, long want) -> int {
        RQ_TRY(expect(want));
        RQ_HIP(hipMemcpyAsync(dst, src, want * 4, hipMemcpyDeviceToDevice, st));
        return RQAMD_OK;
    };
    auto bf16copy = [&](bf16_t* dst, long want) -> int {
        RQ_TRY(expect(want));
        return rq_launch_cvt_bf16(src, dst, want, st);
    };
    int rc = RQAMD_OK;
    bool known = true;
    const int vc = h->cfg.vocab_size_cond < 1 ? 1 : h->cfg.vocab_size_cond;
    if (s == "pos_emb_cond") rc = f32copy(h->pos_cond, h->cond_len * E);
    else if (s == "pos_emb_hw") rc = f32copy(h->pos_hw, h->HW * E);
    else if (s == "pos_emb_d") rc = f32copy(h->pos_d, h->D * E);
    else if (s == "cond_emb.weight") rc = f32copy(h->cond_emb, vc * E);
    else if ((s.rfind("input_mlp.", 0) == 0 && !h->in_vq) || (s.rfind("head_mlp.", 0) == 0 && !h->head_vq)) return RQAMD_OK;
    else if (s == "input_mlp.weight") rc = bf16copy(h->w_in, E * h->Din);
    else if (s == "input_mlp.bias") rc = f32copy(h->b_in, E);
    else if (s == "head_mlp.weight") rc = bf16copy(h->w_headin, E * h->Din);
    else if (s == "head_mlp.bias") rc = f32copy(h->b_headin, E);
    else if (s == "classifier.layer_norm.weight") rc = f32copy(h->cls_lnw, E);
    else if (s == "classifier.layer_norm.bias") rc = f32copy(h->cls_lnb, E);
    else if (s == "classifier.linear.weight") {
        if (h->shared_cls) rc = bf16copy(h->w_cls, (long)h->V * E);
        else {      // BatchLinear (primitives.py:96-125): (depth, in = E, out = V) -> per depth [V][E] bf16
            RQ_TRY(expect((long)h->D * E * h->V));
            if (ndim != 3) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_param(%s): BatchLinear weight must be (depth, in, out)", name);
            for (int d = 0; d < h->D && rc == RQAMD_OK; ++d)
                rc = rq_launch_cvt_bf16_transpose(src + (long)d * E * h->V, h->w_cls + (long)d * h->V * E, (int)E, h->V, st);
        }
    }
    else if (s == "classifier.linear.bias") rc = f32copy(h->b_cls, (h->shared_cls ? 1 : (long)h->D) * h->V);
    else if (s == "tok_emb.weight") {
        if (!h->tok_rows) return RQAMD_OK;
        rc = f32copy(h->tok_emb, h->tok_rows * E);
    }
    else if (s == "tok_emb.offsets") return RQAMD_OK;                  // derived from the vocabulary sizes
    else if (s.rfind("cond_classifier.", 0) == 0) {                    // forward()-only head (transformers.py:150-153)
        if (h->cond_len <= 1) return RQAMD_OK;
        if (s == "cond_classifier.layer_norm.weight") rc = f32copy(h->ccls_lnw, E);
        else if (s == "cond_classifier.layer_norm.bias") rc = f32copy(h->ccls_lnb, E);
        else if (s == "cond_classifier.linear.weight") rc = bf16copy(h->w_ccls, (long)vc * E);
        else if (s == "cond_classifier.linear.bias") rc = f32copy(h->b_ccls, vc);
        else return rq_fail(RQAMD_ERR_INVALID, "rqt_set_param: unknown parameter %s", name);
        if (rc != RQAMD_OK) return rc;
        bool dupc = false;
        for (auto& k : h->seen) if (k == s) { dupc = true; break; }
        if (!dupc) { h->seen.push_back(s); h->n_ccls_seen++; }
        return RQAMD_OK;
    }
    else {
        std::vector<RqtLayer>* stack = nullptr;
        size_t off = 0;
        if (s.rfind("body_transformer.blocks.", 0) == 0) { stack = &h->body; off = strlen("body_transformer.blocks."); }
        else if (s.rfind("head_transformer.blocks.", 0) == 0) { stack = &h->head; off = strlen("head_transformer.blocks."); }
        if (!stack) known = false;
        else {
            size_t dot = s.find('.', off);
            int li = atoi(s.substr(off, dot - off).c_str());
            if (dot == std::string::npos || li < 0 || li >= (int)stack->size())
                return rq_fail(RQAMD_ERR_INVALID, "rqt_set_param: bad layer index in %s", name);
            RqtLayer& L = (*stack)[li];
            std::string leaf = s.substr(dot + 1);
            if (leaf == "ln1.weight") rc = f32copy(L.ln1w, E);
            else if (leaf == "ln1.bias") rc = f32copy(L.ln1b, E);
            else if (leaf == "ln2.weight") rc = f32copy(L.ln2w, E);
            else if (leaf == "ln2.bias") rc = f32copy(L.ln2b, E);
            else if (leaf == "attn.query.weight") rc = bf16copy(L.wqkv, E * E);
            else if (leaf == "attn.key.weight") rc = bf16copy(L.wqkv + E * E, E * E);
            else if (leaf == "attn.value.weight") rc = bf16copy(L.wqkv + 2 * E * E, E * E);
            else if (leaf == "attn.query.bias") rc = f32copy(L.bqkv, E);
            else if (leaf == "attn.key.bias") rc = f32copy(L.bqkv + E, E);
            else if (leaf == "attn.value.bias") rc = f32copy(L.bqkv + 2 * E, E);
            else if (leaf == "attn.proj.weight") rc = bf16copy(L.wproj, E * E);
            else if (leaf == "attn.proj.bias") rc = f32copy(L.bproj, E);
            else if (leaf == "mlp.0.weight") rc = bf16copy(L.wfc1, 4 * E * E);
            else if (leaf == "mlp.0.bias") rc = f32copy(L.bfc1, 4 * E);
            else if (leaf == "mlp.2.weight") rc = bf16copy(L.wfc2, 4 * E * E);
            else if (leaf == "mlp.2.bias") rc = f32copy(L.bfc2, E);
            else known = false;
        }
    }
    if (!known) return rq_fail(RQAMD_ERR_INVALID, "rqt_set_param: unknown parameter %s", name);
    if (rc != RQAMD_OK) return rc;
    bool dup = false;
    for (auto& k : h->seen) if (k == s) { dup = true; break; }
    if (!dup) h->seen.push_back(s);
    h->tables_dirty = true;
    return RQAMD_OK;
}

// -------------------------------------------------------------------------------------------------
// images per prefill chunk / workspace rows for a batch of B (text-conditioned models run the cond_len-1 prefix tokens of
// a chunk of images through the body stack at once: rows = images x (cond_len - 1))
static int prefill_chunk(const rqamd_rqt* h, int B) {
    const int P = h->cond_len - 1;
    if (P < 1) return 0;
    int pc = (B > 4096 ? B : 4096) / P;
    if (pc < 1) pc = 1;
    return pc < B ? pc : B;
}

// groups == 0: the plain layout of the KV workspace.  groups > 0 (a shared-prompt call of that many groups): the shared layout
static int ensure_batch(rqamd_rqt* h, int B, int groups = 0) {
    const bool relay = (groups > 0) != (h->kv_groups > 0);      // the other layout: everything is laid out again, for exactly B rows
    if (B <= h->cap && !relay && groups <= h->kv_groups) return RQAMD_OK;
    // Failure-atomic regrowth: the old capacity is dropped BEFORE anything is freed, and the new one is recorded only after
    // every allocation succeeded -- a failed hipMalloc (the KV cache is ~135 GB at B = 8192) leaves the handle empty
    // (cap 0, no graphs), never pointing at freed memory; the caller may retry with a smaller batch.
    if (!relay && B < h->cap) B = h->cap;                          // (more groups only: the rows stay)
    h->cap = 0;
    h->kv_groups = 0;
    h->gvalid = false;
    for (auto& L : h->body) { L.kc = L.vc = nullptr; L.ksc = L.vsc = nullptr; L.kcs = L.vcs = nullptr; }
    for (auto& L : h->head) { L.kc = L.vc = nullptr; L.ksc = L.vsc = nullptr; }
    if (relay) { h->kv.release(); h->kvg.release(); }              // rqamd_rqt_kv_bytes reports what the layout in force needs
    const size_t E = h->E, V = h->V;
    const size_t brows = (size_t)B;
    const size_t prow = (size_t)prefill_chunk(h, B) * (h->cond_len - 1);
    const size_t rows = brows > prow ? brows : prow;              // activation rows (decode step or prefill chunk)
    size_t total = 2 * al(rows * E * 4) + al((size_t)h->max_slabs * rows * E * 4) + al(brows * V * 4) + 2 * al(rows * E * 2) + al(rows * 3 * E * 2)
                   + al(rows * 4 * E * 2) + al(brows * h->Din * 2) + al(brows * h->HW * h->D * 8) + al(brows * h->cond_len * 8) + al(64) + al(64) + al(brows * 4)
                   + al(brows * h->HW * h->D)
                   + 2 * al(brows * 4) + 4 * al(brows * h->D * 4) + al(brows * 8) + 2 * al(brows * h->HW * h->D * 4)
                   + 6 * al((size_t)h->HW * h->D * 4);
    RQ_TRY(h->ws.reserve(total));
    char* p = (char*)h->ws.p;
    auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return (void*)r; };
    h->x = (float*)take(rows * E * 4); h->xh = (float*)take(rows * E * 4);
    h->slabs = (float*)take((size_t)h->max_slabs * rows * E * 4);
    h->logits = (float*)take(brows * V * 4);
    h->y = (bf16_t*)take(rows * E * 2); h->ya = (bf16_t*)take(rows * E * 2);
    h->qkv = (bf16_t*)take(rows * 3 * E * 2); h->hbuf = (bf16_t*)take(rows * 4 * E * 2);
    h->ain = (bf16_t*)take(brows * h->Din * 2);
    h->xs = (int64_t*)take(brows * h->HW * h->D * 8); h->cond = (int64_t*)take(brows * h->cond_len * 8);
    h->st = (int*)take(64); h->rng = (uint64_t*)take(64); h->smp_redo = (int*)take(brows * 4);
    h->keep = (uint8_t*)take(brows * h->HW * h->D);
    h->row_T = (float*)take(brows * 4); h->row_gs = (float*)take(brows * 4);
    h->row_tk = (int*)take(brows * h->D * 4); h->row_tp = (float*)take(brows * h->D * 4);
    h->row_seed = (uint64_t*)take(brows * 8);
    h->row_mp = (float*)take(brows * h->D * 4); h->row_typ = (float*)take(brows * h->D * 4);
    h->logp_draw = (float*)take(brows * h->HW * h->D * 4); h->logp_model = (float*)take(brows * h->HW * h->D * 4);
    {   // one schedule shared by all images: six [HW][D] tables, whatever the batch
        const size_t sb = (size_t)h->HW * h->D * 4;
        rqamd_rqt::SchedTables& t = h->sch_shared;
        t.T = (float*)take(sb); t.tk = (int*)take(sb); t.tp = (float*)take(sb); t.gs = (float*)take(sb); t.mp = (float*)take(sb); t.typ = (float*)take(sb);
    }
    // KV caches: body [rows][nh][Tbody][64] x2 per layer, head Tcap = D
    // (shared layout, bf16 / fp16 only: HW own slots per (row, head); the P prefix slots live once per group in h->kvg)
    const size_t kvb = al(brows * E * (groups > 0 ? h->HW : h->Tbody) * 2), kvh = al(brows * E * h->D * 2);
    // (8-bit keys: half the bytes for K plus one fp32 scale per (row, head, position))
    const size_t kkb = h->kv_int8k ? al(brows * E * h->Tbody) : kvb, ksb = h->kv_int8k ? al(brows * (E / 64) * h->Tbody * 4) : 0;
    const size_t vvb = h->kv_int8v ? kkb : kvb, vsb = h->kv_int8v ? ksb : 0;
    // The KV workspace is uncached device memory (hipDeviceMallocUncached): every line of it is written once and read once per position, GBs
    // apart -- nothing a cache could serve.  On top of the non-temporal loads of the attention kernels: 5.55 -> 5.67-5.76 TB/s on the decode
    // attention, +0.45 % on the whole step at 10752 images, level at 64 / 500 (profiles/r06_kv_uncached_ab.txt).  RQAMD_KV_UNCACHED=0: plain hipMalloc.
    static const bool kv_uncached = !(getenv("RQAMD_KV_UNCACHED") && atoi(getenv("RQAMD_KV_UNCACHED")) == 0);
    RQ_TRY(h->kv.reserve((kkb + ksb + vvb + vsb) * h->body.size() + 2 * kvh * h->head.size(), kv_uncached ? hipDeviceMallocUncached : 0u));
    char* q = (char*)h->kv.p;
    for (auto& L : h->body) {
        L.kc = (bf16_t*)q; q += kkb; L.vc = (bf16_t*)q; q += vvb;
        L.ksc = h->kv_int8k ? (float*)q : nullptr; q += ksb;
        L.vsc = h->kv_int8v ? (float*)q : nullptr; q += vsb;
    }
    for (auto& L : h->head) { L.kc = (bf16_t*)q; q += kvh; L.vc = (bf16_t*)q; q += kvh; L.ksc = L.vsc = nullptr; }
    if (groups > 0) {
        const size_t gb = al((size_t)groups * E * (h->cond_len - 1) * 2);
        RQ_TRY(h->kvg.reserve(2 * gb * h->body.size()));
        char* g = (char*)h->kvg.p;
        for (auto& L : h->body) { L.kcs = (bf16_t*)g; g += gb; L.vcs = (bf16_t*)g; g += gb; }
    }
    h->kv_groups = groups;
    h->cap = B;
    return RQAMD_OK;
}

static int finalize_tables(rqamd_rqt* h, hipStream_t st) {
    if (h->seen.size() - h->n_ccls_seen < h->n_required)
        return rq_fail(RQAMD_ERR_STATE, "rqt: only %zu of %zu parameters set", h->seen.size() - h->n_ccls_seen, h->n_required);
    if (!h->tables_dirty) return RQAMD_OK;
    long n = (long)h->HW * h->E;
    RQ_LAUNCH(bias_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->b_in, (float)h->D, h->pos_hw, h->body_in_bias, h->HW, h->E);
    n = (long)h->D * h->E;
    RQ_LAUNCH(bias_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->b_headin, 1.0f, h->pos_d, h->head_in_bias, h->D, h->E);
    RQ_TRY(rq_check_launch("bias_table_kernel"));
    h->tables_dirty = false;
    h->gvalid = false;
    return RQAMD_OK;
}

// one weight-streaming GEMM of the decode step; returns slab count for partial epilogues
// residual-producing GEMMs (proj, fc2): `resid` non-null asks for the branch to be added into the fp32 residual stream by
// the GEMM's own epilogue, resid = (resid + acc) + resid_bias, when the tile choice needs no K split -- then *n_slabs = 0 and
// the LayerNorm that follows reads the stream only (one fp32 read + the bf16 write instead of stream + slab in, stream + bf16
// out: 41 -> 18 us per call at 10752 rows; the slab round trip through HBM goes away too).  With a K split the partial slabs and
// their reduction in resid_ln stay as they are.  The additions happen in the same order either way: bit-identical results.
static int step_gemm(rqamd_rqt* h, const bf16_t* A, int lda, const bf16_t* W, int M, int N, int K, int epi,
                     const float* bias, const int* bias_step, int bias_stride, void* out, int ldo, int* n_slabs, hipStream_t st,
                     float* resid = nullptr, const float* resid_bias = nullptr) {
    GemmArgs a{};
    a.A = A; a.W = W; a.M = M; a.N = N; a.K = K; a.lda = lda; a.epi = epi; a.gelu_v2 = h->cur_gelu_v2;
    a.bias = bias; a.bias_step = bias_step; a.bias_stride = bias_stride; a.out = out; a.ldo = ldo;
    int bm, bn, sk, gl = 0;
    rq_gemm_pick_tile(M, N, K, epi == EPI_F32_PARTIAL, &bm, &bn, &sk, &gl);
    if (sk > h->max_slabs) sk = h->max_slabs;
    static const bool no_fuse = getenv("RQAMD_NO_FUSE_RESID") != nullptr;      // A/B switch
    if (resid && epi == EPI_F32_PARTIAL && sk == 1 && !no_fuse && (N & 3) == 0 && !(bm == 64 && bn == 32)) {
        a.accum = 1; a.bias = resid_bias; a.out = resid; a.ldo = N;
        sk = 0;                                                              // reported slab count
    }
    a.splitk = sk > 0 ? sk : 1;
    a.glds = gl;
    if (n_slabs) *n_slabs = sk;
    GemmProfile& pf = h->prof;
    if (pf.skip_gemm) return RQAMD_OK;
    if (pf.on) {
        if (pf.used + 2 > pf.ev.size()) {
            for (int i = 0; i < 2; ++i) { hipEvent_t e; RQ_HIP(hipEventCreate(&e)); pf.ev.push_back(e); }
        }
        RQ_HIP(hipEventRecord(pf.ev[pf.used], st));
    }
    RQ_TRY(rq_gemm_launch(a, bm, bn, st));
    if (pf.on) {
        RQ_HIP(hipEventRecord(pf.ev[pf.used + 1], st));
        pf.used += 2;
        pf.bytes += (double)N * K * 2 + (double)M * K * 2 + (double)M * N * (epi >= EPI_F32 ? 4.0 * (sk > 0 ? sk : 2) : 2.0);
        pf.flops += 2.0 * M * N * K;
    }
    return RQAMD_OK;
}

struct Pending { const float* slabs; int n; const float* bias; };   // un-reduced output of the previous GEMM

// one transformer block on `rows` single-token rows; x is the fp32 residual stream (updated lazily:
// `pend` carries the previous block's fc2 partials + bias into this block's first resid_ln)
struct PrefillCtx { int img0, n_img, P; bool group = false; int T0 = 0; };   // non-null: `rows` = n_img * P prefix tokens of images img0.. (multi-token causal attention)
// T0 > 0 (run_prefill): the P tokens extend caches that hold rows 0 .. T0-1 (rq_launch_attn_extend: head size 64, bf16 / fp16 cache)
// group (a shared-prompt call): the "images" are groups and their keys / values go to the group caches (L.kcs / L.vcs, capacity P = Tcap)
// one-pass forward, non-null: `rows` = n_seq sequences of T consecutive rows, causal attention inside each, no KV cache.
// packed: the head stack's depth groups (T <= 8, a lane per query); else the body stack's (image, token) rows (a lane per query of a
// wavefront per (image, head), K / V staged in LDS)
struct OnePassCtx { int n_seq, T; bool packed; };

static int run_block(rqamd_rqt* h, RqtLayer& L, float* x_in, float* x, Pending& pend, const float* addvec, int rows,
                     const int* step, int step_off, int t_max, int Tcap, hipStream_t st, const PrefillCtx* pf = nullptr,
                     const OnePassCtx* op = nullptr) {
    const int E = h->E;
    ResidLnArgs r{};
    r.x_in = x_in; r.slabs = pend.slabs; r.n_slabs = pend.n; r.bias = pend.bias; r.addvec = addvec;
    r.x_out = (x_in != x || pend.slabs || pend.bias || addvec) ? x : nullptr;      // nothing to add in place: the stream is not rewritten
    r.gamma = L.ln1w; r.beta = L.ln1b; r.y = h->y; r.rows = rows; r.E = E; r.eps = 1e-5f;
    RQ_TRY(rq_launch_resid_ln(r, st));
    RQ_TRY(step_gemm(h, h->y, E, L.wqkv, rows, 3 * E, E, EPI_BF16, L.bqkv, nullptr, 0, h->qkv, 3 * E, nullptr, st));
    if (op && op->packed) {
        AttnPackedArgs ak{};
        ak.qkv = h->qkv; ak.y = h->ya; ak.rows = rows; ak.group = op->T; ak.nh = L.nh; ak.E = E;
        RQ_TRY(rq_launch_attn_packed(ak, st));
    } else if (op) {
        AttnPrefillArgs ap{};                      // kc == null: the cache-free form
        ap.qkv = h->qkv; ap.y = h->ya; ap.n_img = op->n_seq; ap.P = op->T; ap.nh = L.nh; ap.E = E; ap.Tcap = op->T;
        RQ_TRY(rq_launch_attn_prefill(ap, st));
    } else if (pf && pf->T0 > 0) {
        AttnExtendArgs ae{};
        const long img_stride = (long)E * Tcap;
        ae.qkv = h->qkv; ae.y = h->ya; ae.kc = L.kc + pf->img0 * img_stride; ae.vc = L.vc + pf->img0 * img_stride;
        ae.n_img = pf->n_img; ae.R = pf->P; ae.T0 = pf->T0; ae.nh = L.nh; ae.E = E; ae.Tcap = Tcap;
        RQ_TRY(rq_launch_attn_extend(ae, st));
    } else if (pf) {
        AttnPrefillArgs ap{};
        const long img_stride = (long)E * Tcap;
        ap.qkv = h->qkv; ap.y = h->ya;
        ap.vc = L.vsc ? (bf16_t*)((unsigned char*)L.vc + pf->img0 * img_stride) : L.vc + pf->img0 * img_stride;
        ap.vsc = L.vsc ? L.vsc + (long)pf->img0 * L.nh * Tcap : nullptr;
        // (8-bit keys: a key is 64 bytes, i.e. half the bf16 stride, and has one scale)
        ap.kc = L.ksc ? (bf16_t*)((unsigned char*)L.kc + pf->img0 * img_stride) : L.kc + pf->img0 * img_stride;
        ap.ksc = L.ksc ? L.ksc + (long)pf->img0 * L.nh * Tcap : nullptr;
        if (pf->group) { ap.kc = L.kcs + pf->img0 * img_stride; ap.vc = L.vcs + pf->img0 * img_stride; ap.ksc = ap.vsc = nullptr; }
        ap.n_img = pf->n_img; ap.P = pf->P; ap.nh = L.nh; ap.E = E; ap.Tcap = Tcap;
        RQ_TRY(rq_launch_attn_prefill(ap, st));
    } else {
        GemmProfile& pfl = h->prof;
        if (pfl.on) {
            if (pfl.used_attn + 2 > pfl.ev_attn.size())
                for (int i = 0; i < 2; ++i) { hipEvent_t e; RQ_HIP(hipEventCreate(&e)); pfl.ev_attn.push_back(e); }
            RQ_HIP(hipEventRecord(pfl.ev_attn[pfl.used_attn], st));
        }
        if (L.kcs) {
            // shared-prompt layout (body layers only): the prefix keys come from the group's one copy; the own caches hold HW slots per row (run_block's `Tcap` is
            // not used here)
            AttnSharedArgs as{};
            as.qkv = h->qkv; as.kcs = L.kcs; as.vcs = L.vcs; as.kc = L.kc; as.vc = L.vc; as.y = h->ya; as.step = step; as.step_off = step_off;
            as.t_max = t_max; as.rows = rows; as.fan = h->cur_fan; as.nh = L.nh; as.E = E; as.Ps = h->cond_len - 1; as.Tcap = h->HW;
            RQ_TRY(rq_launch_attn_shared(as, st));
        } else {
            AttnDecodeArgs at{};
            at.qkv = h->qkv; at.kc = L.kc; at.vc = L.vc; at.ksc = L.ksc; at.vsc = L.vsc; at.y = h->ya; at.step = step; at.step_off = step_off;
            at.t_max = t_max; at.rows = rows; at.nh = L.nh; at.E = E; at.Tcap = Tcap;
            RQ_TRY(rq_launch_attn_decode(at, st));
        }
        if (pfl.on) { RQ_HIP(hipEventRecord(pfl.ev_attn[pfl.used_attn + 1], st)); pfl.used_attn += 2; }
    }
    int ns = 1;
    RQ_TRY(step_gemm(h, h->ya, E, L.wproj, rows, E, E, EPI_F32_PARTIAL, nullptr, nullptr, 0, h->slabs, E, &ns, st, x, L.bproj));
    ResidLnArgs r2{};
    r2.x_in = x; r2.x_out = ns ? x : nullptr; r2.slabs = ns ? h->slabs : nullptr; r2.n_slabs = ns; r2.bias = ns ? L.bproj : nullptr;
    r2.gamma = L.ln2w; r2.beta = L.ln2b; r2.y = h->y; r2.rows = rows; r2.E = E; r2.eps = 1e-5f;
    RQ_TRY(rq_launch_resid_ln(r2, st));
    RQ_TRY(step_gemm(h, h->y, E, L.wfc1, rows, 4 * E, E, EPI_BF16_GELU, L.bfc1, nullptr, 0, h->hbuf, 4 * E, nullptr, st));
    RQ_TRY(step_gemm(h, h->hbuf, 4 * E, L.wfc2, rows, E, 4 * E, EPI_F32_PARTIAL, nullptr, nullptr, 0, h->slabs, E, &ns, st, x, L.bfc2));
    if (ns) { pend.slabs = h->slabs; pend.n = ns; pend.bias = L.bfc2; }
    else pend = Pending{nullptr, 0, nullptr};      // the stream already holds this block's output
    return RQAMD_OK;
}

struct StepCtx {
    int B;
    const float* const* codebooks;
    float temperature;
    const int* top_k;
    const float* top_p;
    bool sample;           // run the sampler (else teacher-forced)
    const uint8_t* keep;   // sampling: per-code keep flags (h->keep) of a masked call, or null
    bool guided;           // guided sampling: B = 2 * Bs rows run up to the classifier (rows Bs.. are the unconditional twins of rows
    int Bs;                //   0..Bs-1); the sampler runs over Bs rows, mixes the two logits rows of a pair and writes the code to both
    float gscale;
    bool per_row;          // rqamd_rqt_sample_rows: the sampler reads temperature / top_k / top_p (and gscale when guided) of each row from
    bool row_seeds;        //   h->row_*, and with row_seeds the Philox key from h->row_seed; the scalars above are unused
    bool logp;             // armed call (rqamd_rqt_sample_logp): the LOGP samplers write h->logp_draw, a step log_prob launch h->logp_model
    bool trunc;            // min-p / typical sampling in effect (rqamd_rqt_sample_trunc): scalar calls read min_p[d] / typical_p[d] (host arrays of
    const float* min_p;    //   D values, off values where a filter is not given: a depth with both off launches what it launches unarmed); per-row
    const float* typical_p; //  calls read h->row_mp / h->row_typ at every depth
    bool sched;            // scheduled call (rqamd_rqt_sample_schedule): the scheduled per-row samplers read EVERY parameter at (row, position, depth) from
    bool sched_per_image;  //   h->sch_image (a schedule per image) or h->sch_shared (one for all rows); trunc: the min-p / typical tables are read too
    int n_extra;           // composed call (rqamd_rqt_sample_compose): K extra row blocks behind the twins, B = (2 + K) * Bs rows; 0: none
    const int64_t* const* extra_cond;   //   their conditionings (Bs rows each, null entries: zeros)
    bool anchor;           // anchored call (rqamd_rqt_sample_anchor): residual, distance and fold launches per head step (rqt_anchor.hip), the sampler
                           //   reads the scratch; h->anc_w holds a weight per (image, position, depth) whatever the arming gave
    const float* const* acb;   // its codebooks and norms (D device pointers each) and the width of z
    const float* const* acn;
    int adim;
    int fan;               // shared-prompt call (rqamd_rqt_sample_shared): rows per group, `cond` / `uncond` hold B / fan (guided: Bs / fan) rows; 0: a plain call
    float* logits_out;     // teacher-forced: (B,HW,D,V)
    float* cond_logits_out; // teacher-forced, text-conditioned: (B, cond_len-1, vocab_size_cond) or null
};

// body stack for the token whose input is already in h->x; leaves the last fc2 un-reduced in `pend`
// t_max: host-side bound on the number of cached keys (selects the attention kernel's register-block count)
static int body_stack(rqamd_rqt* h, int rows, const int* step, int step_off, int t_max, Pending& pend, hipStream_t st) {
    pend = Pending{nullptr, 0, nullptr};
    h->cur_gelu_v2 = h->cfg.gelu_v2 == 1 || h->cfg.gelu_v2 == 3;
    for (auto& L : h->body) RQ_TRY(run_block(h, L, h->x, h->x, pend, nullptr, rows, step, step_off, t_max, h->Tbody, st));
    return RQAMD_OK;
}

static int embed_gemm(rqamd_rqt* h, const StepCtx& c, int pos_off, int depth_lo, int n_depth, const bf16_t* W, const float* bias_tab,
                      int bias_row_off, bool bias_by_pos, float* out, hipStream_t st) {
    EmbedTokArgs e{};
    e.xs = h->xs; e.pos = h->st; e.pos_off = pos_off; e.depth_lo = depth_lo; e.n_depth = n_depth; e.rows = c.B; e.HW = h->HW; e.D = h->D; e.dim = h->Din;
    e.out = h->ain;
    for (int d = 0; d < h->D; ++d) { e.cb[d] = c.codebooks[d]; e.K[d] = h->Vd[d]; }
    RQ_TRY(rq_launch_embed_tokens(e, st));
    return step_gemm(h, h->ain, h->Din, W, c.B, h->E, h->Din, EPI_F32, bias_tab + (long)bias_row_off * h->E,
                     bias_by_pos ? h->st : nullptr, h->E, out, h->E, nullptr, st);
}

// learned token embeddings (tok_emb) summed over depths [d_lo, d_hi) of the codes at position *st + pos_off, + a positional row
static int tok_embed(rqamd_rqt* h, const StepCtx& c, int pos_off, int d_lo, int d_hi, const float* add, bool add_by_pos, int add_row,
                     float* out, hipStream_t st) {
    TokEmbedArgs t{};
    t.xs = h->xs; t.table = h->tok_emb; t.pos = h->st; t.pos_off = pos_off; t.d_lo = d_lo; t.d_hi = d_hi; t.add = add;
    t.add_by_pos = add_by_pos ? 1 : 0; t.add_row = add_row; t.rows = c.B; t.HW = h->HW; t.D = h->D; t.E = h->E; t.out = out;
    for (int d = 0; d < h->D; ++d) { t.offs[d] = h->tok_offs[d]; t.V[d] = h->Vd[d]; }
    return rq_launch_tok_embed(t, st);
}

// body half of one spatial position (position read from h->st[0] on the device): token embedding + body stack; the last
// fc2 stays un-reduced in `pend`
static int position_body(rqamd_rqt* h, const StepCtx& c, bool first_pos, int host_pos, Pending& pend, hipStream_t st) {
    const int E = h->E, B = c.B;
    if (first_pos) {
        RQ_TRY(rq_launch_cond_embed(h->cond, h->cond_len, h->cond_len - 1, h->cond_emb, h->cfg.vocab_size_cond < 1 ? 1 : h->cfg.vocab_size_cond,
                                    h->pos_cond, h->x, B, E, st));
    } else {
        // token = sum_d input_mlp(e_d) + pos_emb_hw[pos-1]  (transformers.py:218-225), or sum_d tok_emb(code_d) + pos_emb_hw[pos-1]
        if (h->in_vq) RQ_TRY(embed_gemm(h, c, -1, 0, h->D, h->w_in, h->body_in_bias, -1, true, h->x, st));
        else RQ_TRY(tok_embed(h, c, -1, 0, h->D, h->pos_hw, true, -1, h->x, st));
    }
    // a captured graph serves every position of the same 8-key bucket: bound t by the bucket's last position.  Beyond the last bucket
    // (256 tokens and more) one launch sequence serves every later position: the chunked attention kernel's trip count follows the device counter
    const int t_host = host_pos + h->cond_len - 1;
    return body_stack(h, B, h->st, h->cond_len - 1, t_host >= 8 * (rqamd_rqt::NGRAPH - 1) ? h->Tbody - 1 : (t_host | 7), pend, st);
}

// head half: depth d of the position -- head stack, classifier, then the sampler / the teacher-forced copy / nothing
// (stepping form: the caller reads h->logits).  `pend`: the body's pending fc2 (used by d == 0 only).
static int position_depth(rqamd_rqt* h, const StepCtx& c, int d, const Pending& pend, int host_pos, bool mask_only, hipStream_t st) {
    const int E = h->E, B = c.B;
    Pending hp;
    const float* addvec = nullptr;
    float* x_in = h->xh;
    if (d == 0) {
        // head token 0 = spatial context + pos_emb_d[0]; the context is body x + last fc2 (+bias)
        hp = pend; addvec = h->pos_d; x_in = h->x;
    } else {
        // head token d = head_mlp(cumsum_{j<d} e_j) + pos_emb_d[d]  (transformers.py:249-267); without cumsum_depth_ctx only
        // e_{d-1}; with head_emb_vqvae off tok_emb(code_{d-1}) + pos_emb_d[d]
        if (h->head_vq) RQ_TRY(embed_gemm(h, c, 0, h->cumsum ? 0 : d - 1, d, h->w_headin, h->head_in_bias, d, false, h->xh, st));
        else RQ_TRY(tok_embed(h, c, 0, d - 1, d, h->pos_d, false, d, h->xh, st));
        hp = Pending{nullptr, 0, nullptr};
    }
    h->cur_gelu_v2 = h->cfg.gelu_v2 == 1 || h->cfg.gelu_v2 == 2;
    for (size_t li = 0; li < h->head.size(); ++li) {
        RQ_TRY(run_block(h, h->head[li], li == 0 ? x_in : h->xh, h->xh, hp, li == 0 ? addvec : nullptr, B, nullptr, d, d, h->D, st));
    }
    ResidLnArgs r{};
    r.x_in = h->xh; r.x_out = nullptr; r.slabs = hp.slabs; r.n_slabs = hp.n; r.bias = hp.bias;
    if (h->head.empty()) { r.x_in = x_in; r.addvec = addvec; }     // no head stack: the classifier sees the head token itself
    r.gamma = h->cls_lnw; r.beta = h->cls_lnb; r.y = h->y; r.rows = B; r.E = E; r.eps = 1e-5f;
    RQ_TRY(rq_launch_resid_ln(r, st));
    // shared classifier, or BatchLinear's matrix of this depth
    const long cls_off = h->shared_cls ? 0 : (long)d * h->V;
    RQ_TRY(step_gemm(h, h->y, E, h->w_cls + cls_off * E, B, h->V, E, EPI_F32, h->b_cls + cls_off, nullptr, 0, h->logits, h->V, nullptr, st));
    if (c.sample || mask_only) {
        // LogitMask (primitives.py:78-93): codes beyond this depth's vocabulary cannot be drawn.  (The reference's teacher-
        // forced logits are NOT masked -- its mask indexes the wrong axis there -- so rqamd_rqt_logits leaves them alone.)
        if (h->Vd[d] < h->V) RQ_TRY(rq_launch_mask_logits(h->logits, B, h->V, h->Vd[d], st));
    }
    if (c.sample) {
        SampleArgs s{};
        s.logits = h->logits; s.rows = B; s.V = h->V; s.temperature = c.temperature; s.top_k = c.top_k[d]; s.top_p = c.top_p[d];
        s.redo = h->smp_redo; s.rng = h->rng; s.pos = h->st; s.d = d; s.D = h->D; s.out = h->xs; s.out_stride = (long)h->HW * h->D;
        s.keep = c.keep; s.keep_stride = s.out_stride;
        if (c.guided) { s.rows = c.Bs; s.logits_u = h->logits + (long)c.Bs * h->V; s.gscale = c.gscale; s.out_mirror = (long)c.Bs * s.out_stride; }
        if (c.n_extra) {
            // composed guidance: the K extra blocks are folded into the pair (c', u' -> the scratch; h->logits stays raw for the step's
            // log_prob launch), the sampler reads the pair from there and writes the code to all K + 2 rows of the image
            ComposeArgs f{};
            f.c = h->logits; f.u = s.logits_u; f.x = h->logits + 2 * (long)c.Bs * h->V; f.w = h->cmp_w; f.rows = c.Bs; f.V = h->V; f.K = c.n_extra;
            f.out_c = h->cmp_logits; f.out_u = h->cmp_logits + (long)c.Bs * h->V; f.scale = 1.f;
            RQ_TRY(rq_launch_compose(f, st));
            s.logits = f.out_c; s.logits_u = f.out_u; s.out_mirror_n = c.n_extra;
        }
        if (c.anchor) {
            // anchored sampling: the residual of every image at this depth from z and the codes of the position so far, its distances to
            // the codebook of the depth, and the fold of both twins into the scratch (h->logits stays raw for the step's log_prob launch)
            const int n = c.guided ? c.Bs : B;
            AnchorResidArgs r{};
            r.z = h->anc_z; r.z_stride = (long)h->HW * c.adim; r.codes = h->xs; r.code_stride = (long)h->HW * h->D; r.code_D = h->D; r.pos = h->st;
            r.K = h->V; r.d = d; r.dim = c.adim; r.rows = n; r.out = h->anc_resid;
            for (int j = 0; j < d; ++j) r.cb[j] = c.acb[j];
            AnchorFoldArgs f{};
            f.c = s.logits; f.u = c.guided ? s.logits_u : nullptr; f.dist = h->anc_dist; f.w = h->anc_w;
            f.w_row_stride = (long)h->HW * h->D; f.pos = h->st; f.D = h->D; f.d = d; f.rows = n; f.V = h->V;
            f.out_c = h->anc_logits; f.out_u = c.guided ? h->anc_logits + (long)n * h->V : nullptr;
            RQ_TRY(rq_launch_anchor_step(r, c.acb[d], c.acn[d], h->anc_dist, h->anc_pv, h->anc_pi, f, st));
            s.logits = f.out_c; s.logits_u = f.out_u;
        }
        if (c.sched) {         // every value from the tables of the schedule, at (row, *st, d); the scalars are unused
            const rqamd_rqt::SchedTables& t = c.sched_per_image ? h->sch_image : h->sch_shared;
            s.temperature = 1.f; s.top_k = 0; s.top_p = -1.f;
            s.sched = 1; s.row_stride = c.sched_per_image ? (long)h->HW * h->D : 0;
            s.row_temperature = t.T; s.row_top_k = t.tk; s.row_top_p = t.tp;
            s.row_gscale = c.guided ? t.gs : nullptr;
            if (c.row_seeds) { s.row_seeds = h->row_seed; s.rng = nullptr; }
            if (c.trunc) { s.row_min_p = t.mp; s.row_typical_p = t.typ; }
        } else if (c.per_row) {       // rows 0 .. Bs-1 of the tables, for both twins of a guided pair
            s.temperature = 1.f; s.top_k = 0; s.top_p = -1.f;
            s.row_temperature = h->row_T; s.row_top_k = h->row_tk; s.row_top_p = h->row_tp;
            s.row_gscale = c.guided ? h->row_gs : nullptr;
            if (c.row_seeds) { s.row_seeds = h->row_seed; s.rng = nullptr; }      // key row_seed[b], counter 0 + slot (s.offset is 0)
        }
        if (c.logp) s.logp_out = h->logp_draw;
        if (c.trunc && !c.sched) {
            if (c.per_row) { s.row_min_p = h->row_mp; s.row_typical_p = h->row_typ; }
            else { s.min_p = c.min_p[d]; s.typical_p = c.typical_p[d]; }
        }
        RQ_TRY(rq_launch_sample(s, st));
        if (c.logp) {
            // log_softmax(raw logits of the row)[code] for every row of the step (both twins of a guided pair), drawn and kept codes alike:
            // the logits the sampler saw, before guidance and temperature, LogitMask columns at -inf
            LogProbArgs lp{};
            lp.logits = h->logits; lp.ld = h->V; lp.rows = B; lp.V = h->V; lp.targets = h->xs; lp.t_per = 1; lp.t_stride = h->HW * h->D;
            lp.out = h->logp_model; lp.pos = h->st; lp.slot_D = h->D; lp.slot_d = d;
            RQ_TRY(rq_launch_log_prob(lp, st));
        }
    } else if (c.logits_out) {
        float* dst = c.logits_out + ((long)host_pos * h->D + d) * h->V;
        RQ_HIP(hipMemcpy2DAsync(dst, (size_t)h->HW * h->D * h->V * 4, h->logits, (size_t)h->V * 4, (size_t)h->V * 4, B,
                                hipMemcpyDeviceToDevice, st));
    }
    return RQAMD_OK;
}

// the graph family of a sampling call (rqamd_rqt::gkey): scalar and per-row calls 0 .. 23, scheduled calls from NFAM_SCHED0 on
static int step_family(const StepCtx& c) {
    if (c.sched)
        return rqamd_rqt::NFAM_SCHED0 + (c.trunc ? 16 : 0) + (c.logp ? 8 : 0) + (c.row_seeds ? 4 : 0) + (c.sched_per_image ? 2 : 0) + (c.guided ? 1 : 0);
    return (c.trunc ? 12 : 0) + (c.logp ? 6 : 0) + (c.per_row ? (c.row_seeds ? 4 : 2) : 0) + (c.guided ? 1 : 0);
}

// the key / graph-set family of a call: shared-prompt calls have every family of step_family once more
// (composed calls a third time and anchored calls a fourth; a call is only ever one of the three)
static int graph_family(const StepCtx& c) {
    return step_family(c) + (c.fan ? rqamd_rqt::NFAM : c.n_extra ? 2 * rqamd_rqt::NFAM : c.anchor ? 3 * rqamd_rqt::NFAM : 0);
}

// everything that happens at one spatial position (position read from h->st[0] on the device)
static int position_sequence(rqamd_rqt* h, const StepCtx& c, bool first_pos, bool do_head, int host_pos, hipStream_t st) {
    Pending pend;
    RQ_TRY(position_body(h, c, first_pos, host_pos, pend, st));
    if (!do_head) return RQAMD_OK;                 // (the next position overwrites h->x)
    for (int d = 0; d < h->D; ++d) RQ_TRY(position_depth(h, c, d, pend, host_pos, false, st));
    return RQAMD_OK;
}

// inputs into the workspace, position counter to 0, conditioning prefix through the body stack
// (guided sampling: `partial` and `cond` / `uncond` hold c.Bs rows each -- the codes go into both halves of h->xs, the two conditionings
// into the two halves of h->cond)
// skip_text: the caller runs the conditioning prefix itself, merged with the given code positions (prefix_prefill)
static int begin_batch(rqamd_rqt* h, const StepCtx& c, const int64_t* partial, const int64_t* cond, hipStream_t st, const int64_t* uncond = nullptr,
                       bool skip_text = false) {
    const int B = c.B;
    h->step_on = false;                            // any new batch ends a stepping sequence (same workspace)
    const int n_in = c.guided ? c.Bs : B;          // rows the caller gave
    const int n_grp = c.fan ? n_in / c.fan : 0;    // shared-prompt call: rows of `cond` / `uncond`; the prefix runs over n_grp (guided: 2 n_grp) groups
    const int groups = c.guided ? 2 * n_grp : n_grp;
    RQ_TRY(ensure_batch(h, B, groups));
    RQ_TRY(finalize_tables(h, st));
    h->cur_fan = c.fan;
    const size_t xb = (size_t)n_in * h->HW * h->D * 8, cb = (size_t)(c.fan ? n_grp : n_in) * h->cond_len * 8;
    RQ_HIP(hipMemcpyAsync(h->xs, partial, xb, hipMemcpyDeviceToDevice, st));
    if (c.fan) {
        // Shared-prompt call: h->cond holds one row per group first (cond, then uncond) and the P text tokens of the `groups` groups go
        // through the body stack into the group caches -- the loop below over groups instead of rows, capacity P.  Then h->cond is
        // filled again with a row per engine row, for the token of position 0 (position_body).
        const int P = h->cond_len - 1, vc = h->cfg.vocab_size_cond < 1 ? 1 : h->cfg.vocab_size_cond;
        if (cond) RQ_HIP(hipMemcpyAsync(h->cond, cond, cb, hipMemcpyDeviceToDevice, st));
        else RQ_HIP(hipMemsetAsync(h->cond, 0, cb, st));
        if (c.guided) {
            if (uncond) RQ_HIP(hipMemcpyAsync(h->cond + (size_t)n_grp * h->cond_len, uncond, cb, hipMemcpyDeviceToDevice, st));
            else RQ_HIP(hipMemsetAsync(h->cond + (size_t)n_grp * h->cond_len, 0, cb, st));
            RQ_HIP(hipMemcpyAsync(h->xs + (size_t)n_in * h->HW * h->D, partial, xb, hipMemcpyDeviceToDevice, st));
        }
        RQ_TRY(rq_launch_set_int(h->st, 0, st));
        const int pc = prefill_chunk(h, groups);
        for (int b0 = 0; b0 < groups; b0 += pc) {
            PrefillCtx pf{b0, groups - b0 < pc ? groups - b0 : pc, P, true};
            RQ_TRY(rq_launch_cond_embed_multi(h->cond + (long)b0 * h->cond_len, h->cond_len, P, h->cond_emb, vc, h->pos_cond, h->x, pf.n_img, h->E, st));
            Pending pend{nullptr, 0, nullptr};
            h->cur_gelu_v2 = h->cfg.gelu_v2 == 1 || h->cfg.gelu_v2 == 3;
            for (auto& L : h->body) RQ_TRY(run_block(h, L, h->x, h->x, pend, nullptr, pf.n_img * P, nullptr, 0, 0, P, st, &pf));
        }
        const size_t rb = (size_t)n_in * h->cond_len * 8;
        const long nw = (long)n_in * h->cond_len;
        const int64_t* src[2] = {cond, c.guided ? uncond : nullptr};
        for (int half = 0; half < (c.guided ? 2 : 1); ++half) {
            int64_t* dst = h->cond + (size_t)half * n_in * h->cond_len;
            if (src[half]) RQ_LAUNCH(repeat_rows_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, src[half], dst, (long)n_in, h->cond_len, c.fan);
            else RQ_HIP(hipMemsetAsync(dst, 0, rb, st));
        }
        return rq_check_launch("repeat_rows_kernel");
    }
    if (cond) RQ_HIP(hipMemcpyAsync(h->cond, cond, cb, hipMemcpyDeviceToDevice, st));
    else RQ_HIP(hipMemsetAsync(h->cond, 0, cb, st));
    if (c.guided) {
        RQ_HIP(hipMemcpyAsync(h->xs + (size_t)n_in * h->HW * h->D, partial, xb, hipMemcpyDeviceToDevice, st));
        if (uncond) RQ_HIP(hipMemcpyAsync(h->cond + (size_t)n_in * h->cond_len, uncond, cb, hipMemcpyDeviceToDevice, st));
        else RQ_HIP(hipMemsetAsync(h->cond + (size_t)n_in * h->cond_len, 0, cb, st));
        for (int k = 0; k < c.n_extra; ++k) {      // composed call: block 2 + k starts from the same codes, under the k-th extra conditioning
            RQ_HIP(hipMemcpyAsync(h->xs + (size_t)(2 + k) * n_in * h->HW * h->D, partial, xb, hipMemcpyDeviceToDevice, st));
            int64_t* dst = h->cond + (size_t)(2 + k) * n_in * h->cond_len;
            if (c.extra_cond[k]) RQ_HIP(hipMemcpyAsync(dst, c.extra_cond[k], cb, hipMemcpyDeviceToDevice, st));
            else RQ_HIP(hipMemsetAsync(dst, 0, cb, st));
        }
    }
    RQ_TRY(rq_launch_set_int(h->st, 0, st));
    // Conditioning prefix (text tokens): tokens 0..cond_len-2 only fill the body KV cache (transformers.py:235-239; in
    // forward() their body outputs also feed cond_classifier, :150-153).  All P = cond_len-1 tokens of a chunk of images go
    // through the body stack in ONE pass (GEMMs over images x P rows, causal attention inside the prefix), the way the
    // reference's first cached step does -- not as P sequential single-token steps.
    if (h->cond_len > 1 && !skip_text) {
        const int P = h->cond_len - 1, pc = prefill_chunk(h, B), vc = h->cfg.vocab_size_cond < 1 ? 1 : h->cfg.vocab_size_cond;
        for (int b0 = 0; b0 < B; b0 += pc) {
            PrefillCtx pf{b0, B - b0 < pc ? B - b0 : pc, P};
            const int rows = pf.n_img * P;
            RQ_TRY(rq_launch_cond_embed_multi(h->cond + (long)b0 * h->cond_len, h->cond_len, P, h->cond_emb, vc, h->pos_cond, h->x, pf.n_img, h->E, st));
            Pending pend{nullptr, 0, nullptr};
            h->cur_gelu_v2 = h->cfg.gelu_v2 == 1 || h->cfg.gelu_v2 == 3;
            for (auto& L : h->body) RQ_TRY(run_block(h, L, h->x, h->x, pend, nullptr, rows, nullptr, 0, 0, h->Tbody, st, &pf));
            if (c.cond_logits_out) {
                if (!h->w_ccls || h->n_ccls_seen < 4) return rq_fail(RQAMD_ERR_STATE, "rqt: cond_classifier parameters not set");
                ResidLnArgs r{};
                r.x_in = h->x; r.x_out = nullptr; r.slabs = pend.slabs; r.n_slabs = pend.n; r.bias = pend.bias;
                r.gamma = h->ccls_lnw; r.beta = h->ccls_lnb; r.y = h->y; r.rows = rows; r.E = h->E; r.eps = 1e-5f;
                RQ_TRY(rq_launch_resid_ln(r, st));
                RQ_TRY(step_gemm(h, h->y, h->E, h->w_ccls, rows, vc, h->E, EPI_F32, h->b_ccls, nullptr, 0,
                                 c.cond_logits_out + (long)b0 * P * vc, vc, nullptr, st));
            }
        }
    }
    return RQAMD_OK;
}

static int prefix_prefill(rqamd_rqt* h, const float* const* codebooks, int B, int n0, hipStream_t st);
static int run_prefill(rqamd_rqt* h, const float* const* codebooks, int B, int p0, int p1, hipStream_t st);
// can run_prefill serve this handle?  (rq_launch_attn_extend: head size 64 in the body stack, bf16 / fp16 cache; else the run is stepped)
static bool run_prefill_ok(const rqamd_rqt* h) { return !h->kv_int8k && !h->body.empty() && h->E == h->body[0].nh * 64; }

// `keep` / `pos_active` (masked sampling): device flags per code, copied into h->keep before anything reads them, and the host's
// per-position activity (null: every position).  An inactive position has every code given in every row: body stack only, like the
// positions before start_idx.  Nothing runs after the last active position -- nobody reads its KV entries.
static int run_all(rqamd_rqt* h, const StepCtx& c_in, const int64_t* partial, const int64_t* cond, int start_idx, bool use_graph,
                   int64_t* codes_out, hipStream_t st, const uint8_t* keep = nullptr, const uint8_t* pos_active = nullptr,
                   const int64_t* uncond = nullptr, rqamd_rqt::LogpArm arm = {}) {
    StepCtx c = c_in;
    const int n_in = c.guided ? c.Bs : c.B;              // rows of the caller's arrays (guided: the engine runs c.B = 2 * n_in rows)
    int n_pos = h->HW;
    while (keep && pos_active && n_pos > 0 && !pos_active[n_pos - 1]) --n_pos;
    // "prefix.one_pass": n0 = the leading positions whose codes are given in every row (before start_idx, or promised away by pos_active).
    // Their tokens -- and the text tokens before them -- go through the body stack in one pass, and the loop below starts at n0
    int n0 = 0;
    if (h->prefix_one_pass && c.sample && !c.fan)      // (a shared-prompt call steps its code prefix: the text prefix is the shared prefill's)
        while (n0 < n_pos && (n0 < start_idx || (pos_active && !pos_active[n0]))) ++n0;
    RQ_TRY(begin_batch(h, c, partial, cond, st, uncond, n0 >= 1));
    if (keep) {
        const size_t kb = (size_t)n_in * h->HW * h->D;
        RQ_HIP(hipMemcpyAsync(h->keep, keep, kb, hipMemcpyDeviceToDevice, st));
        if (c.guided)                                                                              // (the sampler reads rows 0..Bs-1)
            for (int j = 1; j < 2 + c.n_extra; ++j) RQ_HIP(hipMemcpyAsync(h->keep + (size_t)j * kb, keep, kb, hipMemcpyDeviceToDevice, st));
        c.keep = h->keep;
    }
    if (n0 >= 1 && n0 < n_pos) RQ_TRY(prefix_prefill(h, c.codebooks, c.B, n0, st));      // (n0 == n_pos: no position draws, nothing runs)
    if (c.logp) {          // outside any capture: what no step writes stays +0.0 (draw: kept codes, codes before start_idx) / NaN (model: no head ran)
        const long n = (long)c.B * h->HW * h->D;
        RQ_HIP(hipMemsetAsync(h->logp_draw, 0, (size_t)n * 4, st));
        RQ_LAUNCH(fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->logp_model, __builtin_nanf(""), n);
        RQ_TRY(rq_check_launch("fill_f32_kernel"));
    }
    const int fam = graph_family(c);
    hipGraphExec_t* gexec = h->gexec[2 * fam + (keep ? 1 : 0)];
    // "masked.run_prefill": a run [pos, p1) of positions without a head, behind position 0 and behind the prefix, of two positions at least
    // and with a drawn position after it, goes through the body stack in one pass; the loop goes on at p1.  (A shared-prompt call steps:
    // its own caches begin behind the group's prefix.)
    const bool runs = h->masked_run_prefill && !c.fan && run_prefill_ok(h);
    auto headless = [&](int p) { return !(p >= start_idx && (!pos_active || pos_active[p])); };
    for (int pos = n0; pos < n_pos; ++pos) {
        const bool do_head = !headless(pos);
        if (runs && !do_head && pos >= 1) {
            int p1 = pos + 1;
            while (p1 < n_pos && headless(p1)) ++p1;
            if (p1 - pos >= 2 && p1 < n_pos) {
                RQ_TRY(run_prefill(h, c.codebooks, c.B, pos, p1, st));
                pos = p1 - 1;
                continue;
            }
        }
        const bool graphable = use_graph && c.sample && do_head && pos >= 1 && !h->prof.on;
        if (graphable) {
            if (!h->gvalid) {
                for (auto& set : h->gexec) for (auto& g : set) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
                h->gvalid = true;
                for (auto& f : h->gstale) f = false;
            }
            if (h->gstale[fam]) {                  // this family's key changed: its two sets go, the other family's stay
                for (int f = 2 * fam; f < 2 * fam + 2; ++f) for (auto& g : h->gexec[f]) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
                h->gstale[fam] = false;
            }
            int bucket = (pos + h->cond_len - 1) >> 3;
            if (bucket >= rqamd_rqt::NGRAPH) bucket = rqamd_rqt::NGRAPH - 1;
            if (!gexec[bucket]) {
                hipGraph_t g = nullptr;
                hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
                if (e == hipSuccess) {
                    int rc = position_sequence(h, c, false, true, pos, st);
                    if (rc == RQAMD_OK) rc = rq_launch_add_int(h->st, 1, st);
                    hipError_t e2 = hipStreamEndCapture(st, &g);
                    if (rc != RQAMD_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
                    if (e2 != hipSuccess) return rq_fail(RQAMD_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e2));
                    e2 = hipGraphInstantiate(&gexec[bucket], g, nullptr, nullptr, 0);
                    (void)hipGraphDestroy(g);
                    if (e2 != hipSuccess) return rq_fail(RQAMD_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e2));
                    ++h->n_capture;
                } else {
                    // capture unavailable (e.g. the legacy default stream): eager launches, ~10x the launch count.
                    // Said once, loudly -- this is a performance cliff, not an error.
                    static bool warned = false;
                    if (!warned) { fprintf(stderr, "librqamd: hipStreamBeginCapture failed (%s); sampling runs with eager launches\n", hipGetErrorString(e)); warned = true; }
                    (void)hipGetLastError();
                    use_graph = false;
                }
            }
            if (gexec[bucket]) {
                RQ_HIP(hipGraphLaunch(gexec[bucket], st));
                continue;
            }
        }
        RQ_TRY(position_sequence(h, c, pos == 0, do_head, pos, st));
        RQ_TRY(rq_launch_add_int(h->st, 1, st));
    }
    if (codes_out) RQ_HIP(hipMemcpyAsync(codes_out, h->xs, (size_t)n_in * h->HW * h->D * 8, hipMemcpyDeviceToDevice, st));
    if (c.logp) {
        const size_t lb = (size_t)n_in * h->HW * h->D * 4;
        if (arm.draw) RQ_HIP(hipMemcpyAsync(arm.draw, h->logp_draw, lb, hipMemcpyDeviceToDevice, st));
        if (arm.model) RQ_HIP(hipMemcpyAsync(arm.model, h->logp_model, lb, hipMemcpyDeviceToDevice, st));
        if (arm.model_u) RQ_HIP(hipMemcpyAsync(arm.model_u, h->logp_model + (size_t)n_in * h->HW * h->D, lb, hipMemcpyDeviceToDevice, st));
    }
    return RQAMD_OK;
}

// host arrays of rqamd_rqt_sample_rows (batch rows each; top_k / top_p batch * D)
struct RowParams { const float* temperature; const int* top_k; const float* top_p; const float* gscale; const uint64_t* seeds; };

// the arming of rqamd_rqt_sample_logp, taken by the next sampling call whether it succeeds or fails
static rqamd_rqt::LogpArm take_arm(rqamd_rqt* h) {
    const rqamd_rqt::LogpArm a = h->arm;
    h->arm = {};
    return a;
}
struct ArmGuard {          // an entry point that returns before sample_impl still consumes the armings
    rqamd_rqt* h;
    ~ArmGuard() { if (h) { h->arm = {}; h->tarm = {}; h->sarm = {}; h->shared_fan = 0; h->carm = {}; h->aarm = {}; } }
};

// rqamd_rqt_sample / rqamd_rqt_sample_masked / rqamd_rqt_sample_guided / rqamd_rqt_sample_rows behind their argument checks.  `guided`: `batch` images run as
// 2 * batch engine rows (rows batch.. conditioned on `uncond`), drawn from the guided logits with scale `gscale`
static int sample_impl(rqamd_rqt* h, const int64_t* partial, const uint8_t* keep, const uint8_t* pos_active, const int64_t* cond, int batch,
                       const float* const* codebooks, int start_idx, float temperature, const int* top_k, const float* top_p,
                       uint64_t seed, uint64_t offset, int use_graph, int64_t* codes_out, void* stream,
                       bool guided = false, const int64_t* uncond = nullptr, float gscale = 1.f, const RowParams* rp = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    h->step_on = false;
    const rqamd_rqt::LogpArm arm = take_arm(h);        // (consumed here at the latest: the entry points take it before their own checks)
    const rqamd_rqt::TruncArm tarm = h->tarm;
    h->tarm = {};
    const rqamd_rqt::SchedArm sarm = h->sarm;
    h->sarm = {};
    const int fan = h->shared_fan;
    h->shared_fan = 0;
    const rqamd_rqt::ComposeArm carm = h->carm;
    h->carm = {};
    const rqamd_rqt::AnchorArm aarm = h->aarm;
    h->aarm = {};
    const int K = carm.n;
    const size_t an = (size_t)h->HW * h->D * (aarm.per_image ? (size_t)batch : 1);      // weights of an anchored call
    if (aarm.z) {          // an anchored call (rqamd_rqt_sample_anchor): refused here, before anything is enqueued
        if (aarm.bad) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_anchor: null codebook or norms pointer");
        for (int d = 0; d < h->D; ++d)
            if ((uintptr_t)aarm.cb[d] & 15) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_anchor: codebook %d is not 16-byte aligned", d);
        if (!aarm.weight) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_anchor: null weights");
        if (K) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_anchor: an anchor together with rqamd_rqt_sample_compose");
        if (fan) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_anchor: an anchor together with rqamd_rqt_sample_shared");
        if (aarm.dim % 64 != 0 || aarm.dim < 64 || aarm.dim > 256) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_anchor: dim %d must be 64, 128, 192 or 256", aarm.dim);
        for (int d = 0; d < h->D; ++d)
            if (h->Vd[d] != h->V) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_anchor: depths with different vocabularies (vocab_sizes[%d] = %d < %d)", d, h->Vd[d], h->V);
        for (size_t i = 0; i < an; ++i)
            if (!(aarm.weight[i] >= 0.f) || !(aarm.weight[i] - aarm.weight[i] == 0.f))
                return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_anchor: weight[%zu] must be finite and >= 0", i);
    }
    if (K) {               // a composed call (rqamd_rqt_sample_compose): refused here, before anything is enqueued
        if (!guided) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_compose: extra conditions armed in front of an unguided call");
        if (fan) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_compose: extra conditions together with rqamd_rqt_sample_shared (no group caches for the extra blocks)");
        if (K < 0 || K > RQ_MAX_EXTRA_CONDS) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_compose: %d extra conditions (at most %d)", K, (int)RQ_MAX_EXTRA_CONDS);
        if (!carm.weight) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_compose: null weights");
        if (batch > 0x7fffffff / (2 + K)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_compose: (2 + %d) * batch overflows", K);
        for (long i = 0; i < (long)K * batch; ++i)
            if (!(carm.weight[i] - carm.weight[i] == 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_compose: weight[%ld] must be finite", i);
    }
    if (fan) {             // a shared-prompt call (rqamd_rqt_sample_shared): refused here, before anything is enqueued
        if (fan < 0 || batch % fan) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_shared: batch %d is not a multiple of the group size %d", batch, fan);
        if (h->cfg.block_size_cond < 2) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_shared: block_size_cond = %d: no text prefix to share", h->cfg.block_size_cond);
        if (h->kv_int8k) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_shared: RQAMD_KV=%s (the shared attention reads bf16 / fp16 caches)", h->kv_int8v ? "int8kv" : "int8k");
        if (h->Tbody > 256) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_shared: body context %d > 256", h->Tbody);
        if (h->E != h->cfg.n_head * 64) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_sample_shared: body head size %d (64 only)", h->E / h->cfg.n_head);
    }
    if (arm.model_u && !guided) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_logp: model_logp_uncond_out armed for an unguided call");
    // min-p / typical values of the call: tr_mp / tr_typ hold D values (scalar calls) or batch * D (per-row calls: a D-entry arming is
    // repeated for every image), off values where a filter is not given.  Scalar calls whose every value is off are unarmed calls.
    if (tarm.per_image && !rp) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_trunc: per-image values armed in front of a call without per-row parameters");
    std::vector<float> tr_mp, tr_typ;
    bool trunc = false;
    if (tarm.on()) {
        const size_t n = (rp ? (size_t)batch : 1) * h->D;
        tr_mp.assign(n, 0.f); tr_typ.assign(n, -1.f);
        for (size_t i = 0; i < n; ++i) {
            const size_t j = tarm.per_image ? i : i % h->D;
            if (tarm.min_p) tr_mp[i] = tarm.min_p[j];
            if (tarm.typical_p) tr_typ[i] = tarm.typical_p[j];
            if (!(tr_mp[i] - tr_mp[i] == 0.f) || tr_mp[i] > 1.0f) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_trunc: min_p[%d] must be finite and at most 1", (int)j);
            if (!(tr_typ[i] - tr_typ[i] == 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_trunc: typical_p[%d] must be finite", (int)j);
            if (!(tr_mp[i] > 0.f)) tr_mp[i] = 0.f;                                     // one off value each: equal keys for equal behaviour
            if (!(tr_typ[i] >= 0.f && tr_typ[i] < 1.0f)) tr_typ[i] = -1.f;
            trunc = trunc || tr_mp[i] > 0.f || tr_typ[i] >= 0.f;
        }
        if (rp) trunc = true;          // per-row: the tables are read on the device, whatever they hold
    }
    // a schedule armed by rqamd_rqt_sample_schedule: its values are checked here, before anything is enqueued or written
    const size_t sn = (size_t)h->HW * h->D;
    if (sarm.on()) {
        if (sarm.gscale && !guided) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_schedule: a guidance schedule armed in front of an unguided call");
        const size_t n = (sarm.per_image ? (size_t)batch : 1) * sn;
        for (size_t i = 0; i < n; ++i) {
            if (sarm.temperature && (!(sarm.temperature[i] > 0.f) || !(sarm.temperature[i] - sarm.temperature[i] == 0.f)))
                return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_schedule: temperature[%zu] must be > 0 and finite", i);
            if (sarm.gscale && !(sarm.gscale[i] - sarm.gscale[i] == 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_schedule: guidance_scale[%zu] must be finite", i);
            if (sarm.min_p && (!(sarm.min_p[i] - sarm.min_p[i] == 0.f) || sarm.min_p[i] > 1.0f))
                return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_schedule: min_p[%zu] must be finite and at most 1", i);
            if (sarm.typical_p && !(sarm.typical_p[i] - sarm.typical_p[i] == 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_schedule: typical_p[%zu] must be finite", i);
        }
    }
    const int rows = guided ? (2 + K) * batch : batch;
    RQ_TRY(ensure_batch(h, rows, fan ? rows / fan : 0));
    StepCtx c{};
    c.n_extra = K; c.extra_cond = carm.cond;
    if (K) {
        // the fold's scratch and weight table: first use, or a larger batch, outside any capture -- the composed graphs hold the old addresses.
        // Weights: host array -> staging block of the handle -> device table by an asynchronous copy ahead of the position loop (see row_host)
        if ((size_t)batch > h->cmp_rows) {
            h->cmp_rows = 0;
            const size_t lb = al(2 * (size_t)batch * h->V * 4);
            RQ_TRY(h->cmp_buf.reserve(lb + al((size_t)RQ_MAX_EXTRA_CONDS * batch * 4)));
            h->cmp_logits = (float*)h->cmp_buf.p; h->cmp_w = (float*)((char*)h->cmp_buf.p + lb);
            h->cmp_rows = (size_t)batch;
            for (int f = 2 * rqamd_rqt::NFAM; f < 3 * rqamd_rqt::NFAM; ++f) h->gstale[f] = true;
        }
        RQ_HIP(hipStreamSynchronize(st));
        h->cmp_host.assign(carm.weight, carm.weight + (size_t)K * batch);
        RQ_HIP(hipMemcpyAsync(h->cmp_w, h->cmp_host.data(), (size_t)K * batch * 4, hipMemcpyHostToDevice, st));
    }
    if (aarm.z) {
        // the block of the three launches: first use, a larger batch or a wider z, outside any capture -- the anchored graphs hold the old
        // addresses.  z: device copy on the stream; weights: host array -> staging block of the handle -> device table by an asynchronous
        // copy ahead of the position loop (see row_host)
        const size_t lrows = guided ? 2 * (size_t)batch : (size_t)batch;
        if ((size_t)batch > h->anc_imgs || lrows > h->anc_lrows || (size_t)aarm.dim > h->anc_dim) {
            const size_t ni = std::max(h->anc_imgs, (size_t)batch), nl = std::max(h->anc_lrows, lrows), nd = std::max(h->anc_dim, (size_t)aarm.dim);
            h->anc_imgs = h->anc_lrows = h->anc_dim = 0;
            const size_t bl = al(nl * h->V * 4), bd = al(ni * h->V * 4), br = al(ni * nd * 4), bp = al(ni * 64 * 4), bz = al(ni * h->HW * nd * 4),
                         bw = al(ni * h->HW * h->D * 4);
            RQ_TRY(h->anc_buf.reserve(bl + bd + br + 2 * bp + bz + bw));
            char* q = (char*)h->anc_buf.p;
            h->anc_logits = (float*)q; q += bl;
            h->anc_dist = (float*)q; q += bd;
            h->anc_resid = (float*)q; q += br;
            h->anc_pv = (float*)q; q += bp;
            h->anc_pi = (int*)q; q += bp;
            h->anc_z = (float*)q; q += bz;
            h->anc_w = (float*)q;
            h->anc_imgs = ni; h->anc_lrows = nl; h->anc_dim = nd;
            for (int f = 3 * rqamd_rqt::NFAM; f < 4 * rqamd_rqt::NFAM; ++f) h->gstale[f] = true;
        }
        RQ_HIP(hipStreamSynchronize(st));
        // (one table per image in every case -- a shared table is repeated -- so that the captured fold launches hold ONE row stride and
        //  calls with either kind of table replay the same graphs)
        const size_t sn_w = (size_t)h->HW * h->D;
        h->anc_host.resize((size_t)batch * sn_w);
        for (int b = 0; b < batch; ++b) memcpy(h->anc_host.data() + b * sn_w, aarm.weight + (aarm.per_image ? b * sn_w : 0), sn_w * 4);
        RQ_HIP(hipMemcpyAsync(h->anc_w, h->anc_host.data(), (size_t)batch * sn_w * 4, hipMemcpyHostToDevice, st));
        RQ_HIP(hipMemcpyAsync(h->anc_z, aarm.z, (size_t)batch * h->HW * aarm.dim * 4, hipMemcpyDeviceToDevice, st));
        c.anchor = true; c.acb = aarm.cb; c.acn = aarm.cn; c.adim = aarm.dim;
    }
    c.B = rows; c.codebooks = codebooks; c.temperature = temperature; c.top_k = top_k; c.top_p = top_p; c.sample = true;
    c.fan = fan;
    c.guided = guided; c.Bs = batch; c.gscale = gscale; c.logp = arm.on();
    c.trunc = trunc; c.min_p = tr_mp.data(); c.typical_p = tr_typ.data();
    if (rp) {
        // per-row values: host arrays -> one staging block owned by the handle -> h->row_* by asynchronous copies ahead of the position
        // loop on the same stream, outside any capture.  The caller's arrays are read before this function returns; the staging block
        // is what the copies read, so it is rewritten only once the stream has drained (idle already in the usual case: callers wait
        // for the codes of one call before they make the next).
        c.per_row = true; c.row_seeds = rp->seeds != nullptr;
        const size_t nB = (size_t)batch, nD = nB * h->D;
        const size_t oT = 0, oG = oT + nB * 4, oK = oG + nB * 4, oP = oK + nD * 4, oM = oP + nD * 4, oY = oM + nD * 4, oS = (oY + nD * 4 + 7) & ~(size_t)7, total = oS + nB * 8;
        RQ_HIP(hipStreamSynchronize(st));
        h->row_host.resize(total);
        char* hb = h->row_host.data();
        memcpy(hb + oT, rp->temperature, nB * 4);
        if (guided) memcpy(hb + oG, rp->gscale, nB * 4);
        memcpy(hb + oK, rp->top_k, nD * 4);
        memcpy(hb + oP, rp->top_p, nD * 4);
        if (rp->seeds) memcpy(hb + oS, rp->seeds, nB * 8);
        if (trunc) { memcpy(hb + oM, tr_mp.data(), nD * 4); memcpy(hb + oY, tr_typ.data(), nD * 4); }
        RQ_HIP(hipMemcpyAsync(h->row_T, hb + oT, nB * 4, hipMemcpyHostToDevice, st));
        if (guided) RQ_HIP(hipMemcpyAsync(h->row_gs, hb + oG, nB * 4, hipMemcpyHostToDevice, st));
        RQ_HIP(hipMemcpyAsync(h->row_tk, hb + oK, nD * 4, hipMemcpyHostToDevice, st));
        RQ_HIP(hipMemcpyAsync(h->row_tp, hb + oP, nD * 4, hipMemcpyHostToDevice, st));
        if (rp->seeds) RQ_HIP(hipMemcpyAsync(h->row_seed, hb + oS, nB * 8, hipMemcpyHostToDevice, st));
        if (trunc) {
            RQ_HIP(hipMemcpyAsync(h->row_mp, hb + oM, nD * 4, hipMemcpyHostToDevice, st));
            RQ_HIP(hipMemcpyAsync(h->row_typ, hb + oY, nD * 4, hipMemcpyHostToDevice, st));
        }
    }
    if (sarm.on()) {
        // The tables of the scheduled call: a value for every (image, position, depth) -- or, one schedule for all images and no per-image
        // argument anywhere, for every (position, depth) -- from the schedule where it gives the parameter, else from the call's own
        // arguments, broadcast.  Host staging block -> device tables by asynchronous copies ahead of the position loop, as above.
        const bool pi = sarm.per_image || rp;
        const size_t nimg = pi ? (size_t)batch : 1, nt = nimg * sn;
        const int D = h->D;
        RQ_HIP(hipStreamSynchronize(st));
        h->sch_host.resize(6 * nt * 4);
        float* hT = (float*)h->sch_host.data();
        int* hK = (int*)(hT + nt);
        float *hP = (float*)(hK + nt), *hG = hP + nt, *hM = hG + nt, *hY = hM + nt;
        bool any_trunc = false;
        for (size_t b = 0; b < nimg; ++b) {
            for (size_t q = 0; q < sn; ++q) {
                const size_t i = b * sn + q, j = (sarm.per_image ? b * sn : 0) + q, d = q % D;
                hT[i] = sarm.temperature ? sarm.temperature[j] : rp ? rp->temperature[b] : temperature;
                hK[i] = sarm.top_k ? sarm.top_k[j] : rp ? rp->top_k[b * D + d] : top_k[d];
                hP[i] = sarm.top_p ? sarm.top_p[j] : rp ? rp->top_p[b * D + d] : top_p[d];
                hG[i] = !guided ? 1.f : sarm.gscale ? sarm.gscale[j] : rp ? rp->gscale[b] : gscale;
                float m = sarm.min_p ? sarm.min_p[j] : tr_mp.empty() ? 0.f : tr_mp[(rp ? b * D : 0) + d];
                float y = sarm.typical_p ? sarm.typical_p[j] : tr_typ.empty() ? -1.f : tr_typ[(rp ? b * D : 0) + d];
                if (!(m > 0.f)) m = 0.f;                                   // the off values of the per-row arrays
                if (!(y >= 0.f && y < 1.0f)) y = -1.f;
                hM[i] = m; hY[i] = y;
                any_trunc = any_trunc || m > 0.f || y >= 0.f;
            }
        }
        trunc = any_trunc;             // a filter on somewhere: the TRUNC builds read the two tables; nowhere: the builds without the stages
        if (pi && (size_t)batch > h->sch_image_rows) {
            // first use, or a larger batch: outside any capture.  The graphs of the per-image scheduled families hold the old addresses
            h->sch_image_rows = 0;
            const size_t tb = al((size_t)batch * sn * 4);
            RQ_TRY(h->sch_image_buf.reserve(6 * tb));
            char* q = (char*)h->sch_image_buf.p;
            rqamd_rqt::SchedTables& t = h->sch_image;
            t.T = (float*)q; t.tk = (int*)(q + tb); t.tp = (float*)(q + 2 * tb); t.gs = (float*)(q + 3 * tb); t.mp = (float*)(q + 4 * tb); t.typ = (float*)(q + 5 * tb);
            h->sch_image_rows = (size_t)batch;
            for (int f = rqamd_rqt::NFAM_SCHED0; f < rqamd_rqt::NFAM; ++f)
                if ((f - rqamd_rqt::NFAM_SCHED0) & 2) h->gstale[f] = h->gstale[f + rqamd_rqt::NFAM] = h->gstale[f + 2 * rqamd_rqt::NFAM] = h->gstale[f + 3 * rqamd_rqt::NFAM] = true;
        }
        const rqamd_rqt::SchedTables& t = pi ? h->sch_image : h->sch_shared;
        RQ_HIP(hipMemcpyAsync(t.T, hT, nt * 4, hipMemcpyHostToDevice, st));
        RQ_HIP(hipMemcpyAsync(t.tk, hK, nt * 4, hipMemcpyHostToDevice, st));
        RQ_HIP(hipMemcpyAsync(t.tp, hP, nt * 4, hipMemcpyHostToDevice, st));
        if (guided) RQ_HIP(hipMemcpyAsync(t.gs, hG, nt * 4, hipMemcpyHostToDevice, st));
        if (trunc) {
            RQ_HIP(hipMemcpyAsync(t.mp, hM, nt * 4, hipMemcpyHostToDevice, st));
            RQ_HIP(hipMemcpyAsync(t.typ, hY, nt * 4, hipMemcpyHostToDevice, st));
        }
        c.sched = true; c.sched_per_image = pi; c.trunc = trunc;
        c.row_seeds = rp && rp->seeds;
    }
    // graph cache key: anything baked into kernel arguments (the keep-flag pointer is not in it: masked calls have a graph set of their
    // own).  One key per family: a guided call never invalidates the unguided graphs, nor the other way round
    rqamd_rqt::Key k{};
    k.B = rows; k.guided = guided ? 1 : 0; k.stream = stream; k.fan = fan; k.n_extra = K;
    for (int d = 0; d < h->D; ++d) k.cb[d] = codebooks[d];
    if (aarm.z) {
        for (int d = 0; d < h->D; ++d) { k.acb[d] = aarm.cb[d]; k.acn[d] = aarm.cn[d]; }
        k.adim = aarm.dim;
    }
    if (!rp && !sarm.on()) {       // (per-row and scheduled calls: no parameter value is in a captured launch, so none is in the key)
        k.T = temperature; k.gs = guided ? gscale : 0.f;
        for (int d = 0; d < h->D; ++d) { k.tk[d] = top_k[d]; k.tp[d] = top_p[d]; }
        if (trunc) for (int d = 0; d < h->D; ++d) { k.mp[d] = tr_mp[d]; k.typ[d] = tr_typ[d]; }
    }
    const int fam = graph_family(c);
    if (!h->gkey_set[fam] || memcmp(&k, &h->gkey[fam], sizeof(k)) != 0) { h->gstale[fam] = true; h->gkey[fam] = k; h->gkey_set[fam] = true; }
    RQ_LAUNCH(set_rng_kernel, dim3(1), dim3(64), 0, st, h->rng, seed, offset);
    h->prof.used = 0; h->prof.bytes = 0; h->prof.flops = 0; h->prof.used_attn = 0;
    RQ_TRY(run_all(h, c, partial, cond, start_idx, use_graph != 0, codes_out, st, keep, pos_active, uncond, arm));
    if (h->prof.on) {
        RQ_HIP(hipStreamSynchronize(st));
        double ms = 0;
        for (size_t i = 0; i + 1 < h->prof.used; i += 2) {
            float t = 0.f;
            RQ_HIP(hipEventElapsedTime(&t, h->prof.ev[i], h->prof.ev[i + 1]));
            ms += t;
        }
        h->prof.ms_total = ms;
        h->prof.launches = (int64_t)(h->prof.used / 2);
        ms = 0;
        for (size_t i = 0; i + 1 < h->prof.used_attn; i += 2) {
            float t = 0.f;
            RQ_HIP(hipEventElapsedTime(&t, h->prof.ev_attn[i], h->prof.ev_attn[i + 1]));
            ms += t;
        }
        h->prof.attn_ms_total = ms;
        h->prof.attn_launches = (int64_t)(h->prof.used_attn / 2);
    }
    return RQAMD_OK;
}

extern "C" int rqamd_rqt_sample(rqamd_rqt* h, const int64_t* partial, const int64_t* cond, int batch,
                                const float* const* codebooks, int start_h, int start_w, float temperature,
                                const int* top_k, const float* top_p, uint64_t seed, uint64_t offset,
                                int use_graph, int64_t* codes_out, void* stream) {
    ArmGuard arm_guard{h};
    if (!h || !partial || !codebooks || !top_k || !top_p || !codes_out) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample: null argument");
    if (batch < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample: batch < 1");
    if (!(temperature > 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample: temperature must be > 0");
    int start_idx = start_h * h->cfg.W + start_w;
    if (start_idx < 0) start_idx = 0;
    return sample_impl(h, partial, nullptr, nullptr, cond, batch, codebooks, start_idx, temperature, top_k, top_p, seed, offset, use_graph,
                       codes_out, stream);
}

// Masked form (include/rqamd.h): a kept code stays as `partial` gives it, every other code is drawn exactly as rqamd_rqt_sample draws
// it -- same logits, same filter, same Philox counter offset + pos * D + d of its row -- so a masked call whose kept codes are what
// the unmasked call drew reproduces that call bit for bit.  The sampler kernels skip kept (row, slot)s; everything else is the
// unmasked launch sequence.
extern "C" int rqamd_rqt_sample_masked(rqamd_rqt* h, const int64_t* partial, const uint8_t* keep, const uint8_t* pos_active_host,
                                       const int64_t* cond, int batch, const float* const* codebooks, float temperature,
                                       const int* top_k, const float* top_p, uint64_t seed, uint64_t offset,
                                       int use_graph, int64_t* codes_out, void* stream) {
    ArmGuard arm_guard{h};
    if (!h || !partial || !keep || !codebooks || !top_k || !top_p || !codes_out)
        return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_masked: null argument");
    if (batch < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_masked: batch < 1");
    if (!(temperature > 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_masked: temperature must be > 0");
    return sample_impl(h, partial, keep, pos_active_host, cond, batch, codebooks, 0, temperature, top_k, top_p, seed, offset, use_graph,
                       codes_out, stream);
}

// Guided form (include/rqamd.h): classifier-free guidance inside the engine.  Image b runs twice, as row b under `cond` and as row
// batch + b under `uncond`; at every step the sampler draws row b from guide(logits[b], logits[batch + b], guidance_scale) with the
// filter and the Philox counter of row b of an unguided call, and writes the code to both rows -- the twin sees exactly what was drawn.
extern "C" int rqamd_rqt_sample_guided(rqamd_rqt* h, const int64_t* partial, const uint8_t* keep, const uint8_t* pos_active_host,
                                       const int64_t* cond, const int64_t* uncond, int batch, const float* const* codebooks,
                                       int start_h, int start_w, float temperature, float guidance_scale, const int* top_k,
                                       const float* top_p, uint64_t seed, uint64_t offset, int use_graph, int64_t* codes_out, void* stream) {
    ArmGuard arm_guard{h};
    if (!h || !partial || !codebooks || !top_k || !top_p || !codes_out) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_guided: null argument");
    if (batch < 1 || batch > 0x3fffffff) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_guided: batch < 1 (or 2 * batch overflows)");
    if (!(temperature > 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_guided: temperature must be > 0");
    if (!(guidance_scale - guidance_scale == 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_guided: guidance_scale must be finite");
    int start_idx = start_h * h->cfg.W + start_w;
    if (start_idx < 0) start_idx = 0;
    return sample_impl(h, partial, keep, keep ? pos_active_host : nullptr, cond, batch, codebooks, start_idx, temperature, top_k, top_p, seed,
                       offset, use_graph, codes_out, stream, true, uncond, guidance_scale);
}

// Per-row form (include/rqamd.h): plain, masked and guided sampling with a temperature, top-k, top-p, guidance scale and optionally a
// Philox seed per image.  The launch sequence is that of the scalar forms with the per-row sampler kernels (rqt_sample_rows.hip) in
// place of the scalar ones; row b is drawn exactly as the scalar form with b's values draws it.
extern "C" int rqamd_rqt_sample_rows(rqamd_rqt* h, const int64_t* partial, const uint8_t* keep, const uint8_t* pos_active_host,
                                     const int64_t* cond, const int64_t* uncond, int batch, const float* const* codebooks,
                                     int start_h, int start_w, const float* temperature, const int* top_k, const float* top_p,
                                     const float* guidance_scale, const uint64_t* seeds, uint64_t seed, uint64_t offset,
                                     int use_graph, int64_t* codes_out, void* stream) {
    ArmGuard arm_guard{h};
    if (!h || !partial || !codebooks || !temperature || !top_k || !top_p || !codes_out)
        return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_rows: null argument");
    if (batch < 1 || batch > 0x3fffffff) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_rows: batch < 1 (or 2 * batch overflows)");
    if (uncond && !guidance_scale) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_rows: uncond without guidance_scale (null)");
    const bool guided = guidance_scale != nullptr;
    for (int b = 0; b < batch; ++b) {
        const float t = temperature[b];
        if (!(t > 0.f) || !(t - t == 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_rows: temperature[%d] must be > 0 and finite", b);
        if (guided && !(guidance_scale[b] - guidance_scale[b] == 0.f))
            return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_rows: guidance_scale[%d] must be finite", b);
    }
    int start_idx = start_h * h->cfg.W + start_w;
    if (start_idx < 0) start_idx = 0;
    const RowParams rp{temperature, top_k, top_p, guidance_scale, seeds};
    static const int no_k[8] = {};
    static const float no_p[8] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f};
    return sample_impl(h, partial, keep, keep ? pos_active_host : nullptr, cond, batch, codebooks, start_idx, 1.f, no_k, no_p, seed, offset,
                       use_graph, codes_out, stream, guided, uncond, 1.f, &rp);
}

// Arms the next rqamd_rqt_sample / _masked / _guided / _rows call on the handle (include/rqamd.h): device pointers to (batch, H, W, D)
// fp32 each, any of them NULL, all NULL disarms.  The armed call draws the codes of the unarmed one; its outputs are copied out of
// the handle's workspace next to the codes, so no captured graph ever holds a caller's pointer.
extern "C" int rqamd_rqt_sample_logp(rqamd_rqt* h, float* draw_logp_out, float* model_logp_out, float* model_logp_uncond_out) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_logp: null handle");
    h->arm = rqamd_rqt::LogpArm{draw_logp_out, model_logp_out, model_logp_uncond_out};
    return RQAMD_OK;
}

// Arms the next rqamd_rqt_sample / _masked / _guided / _rows call on the handle with min-p and / or locally typical sampling
// (include/rqamd.h): HOST arrays, read by that call -- D values, or batch * D image-major with per_image = 1 (in front of
// rqamd_rqt_sample_rows only).  Either NULL: that filter is off; both NULL disarms.
extern "C" int rqamd_rqt_sample_trunc(rqamd_rqt* h, const float* min_p, const float* typical_p, int per_image) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_trunc: null handle");
    h->tarm = rqamd_rqt::TruncArm{min_p, typical_p, (min_p || typical_p) && per_image ? 1 : 0};
    return RQAMD_OK;
}

// Arms the next rqamd_rqt_sample / _masked / _guided / _rows call on the handle with sampling schedules over positions and depths
// (include/rqamd.h): HOST arrays of H * W * D values -- batch * H * W * D image-major with per_image = 1 -- read and checked by that
// call, each or NULL (the parameter comes from the call's own arguments); all NULL disarms.
extern "C" int rqamd_rqt_sample_schedule(rqamd_rqt* h, const float* temperature, const int* top_k, const float* top_p,
                                         const float* guidance_scale, const float* min_p, const float* typical_p, int per_image) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_schedule: null handle");
    h->sarm = rqamd_rqt::SchedArm{temperature, top_k, top_p, guidance_scale, min_p, typical_p, 0};
    h->sarm.per_image = h->sarm.on() && per_image ? 1 : 0;
    return RQAMD_OK;
}

// Arms the next rqamd_rqt_sample / _masked / _guided / _rows call on the handle as a shared-prompt call (include/rqamd.h): `fan` rows per
// group, one row of cond / uncond per group.  0 disarms.
extern "C" int rqamd_rqt_sample_shared(rqamd_rqt* h, int fan) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_shared: null handle");
    h->shared_fan = 0;
    if (fan < 0) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_shared: fan = %d < 0", fan);
    h->shared_fan = fan;
    return RQAMD_OK;
}

// Arms the next rqamd_rqt_sample_guided call, or guided rqamd_rqt_sample_rows call, on the handle with extra conditions (include/rqamd.h):
// n_extra device pointers (batch rows of conditioning each, null entries: zeros; the pointer ARRAY is copied here) and HOST weights
// (n_extra * batch, condition-major), read and checked by that call.  0 disarms.
extern "C" int rqamd_rqt_sample_compose(rqamd_rqt* h, int n_extra, const int64_t* const* extra_cond, const float* extra_weight) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_compose: null handle");
    h->carm = {};
    if (n_extra == 0) return RQAMD_OK;
    if (n_extra < 0 || n_extra > RQ_MAX_EXTRA_CONDS)
        return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_compose: %d extra conditions (0 .. RQAMD_RQT_MAX_EXTRA_CONDS = %d)", n_extra, (int)RQ_MAX_EXTRA_CONDS);
    if (!extra_weight) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_compose: null weights");
    h->carm.n = n_extra;
    for (int k = 0; k < n_extra; ++k) h->carm.cond[k] = extra_cond ? extra_cond[k] : nullptr;
    h->carm.weight = extra_weight;
    return RQAMD_OK;
}

// Arms the next rqamd_rqt_sample / _masked / _guided / _rows call on the handle as an anchored call (include/rqamd.h): z (batch, H, W, dim)
// fp32 DEVICE, D DEVICE pointers each to the codebooks (vocab codes of width dim) and their norms (the two pointer ARRAYS are copied
// here), and HOST weights (H * W * D, or batch * H * W * D image-major with per_image = 1), read and checked by that call.  z NULL disarms.
extern "C" int rqamd_rqt_sample_anchor(rqamd_rqt* h, const float* z, const float* const* codebooks, const float* const* code_norms, int dim,
                                       const float* weight, int per_image) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "rqt_sample_anchor: null handle");
    h->aarm = {};
    if (!z) return RQAMD_OK;
    h->aarm.z = z; h->aarm.dim = dim; h->aarm.weight = weight; h->aarm.per_image = per_image ? 1 : 0;
    for (int d = 0; d < h->D; ++d) {
        h->aarm.cb[d] = codebooks ? codebooks[d] : nullptr;
        h->aarm.cn[d] = code_norms ? code_norms[d] : nullptr;
        if (!h->aarm.cb[d] || !h->aarm.cn[d]) h->aarm.bad = 1;      // (refused by the armed call, which consumes the arming)
    }
    return RQAMD_OK;
}

extern "C" int rqamd_rqt_kv_bytes(rqamd_rqt* h, int64_t* bytes) {
    if (!h || !bytes) return rq_fail(RQAMD_ERR_INVALID, "rqt_kv_bytes: null argument");
    *bytes = (int64_t)(h->kv.bytes + h->kvg.bytes);
    return RQAMD_OK;
}

extern "C" int rqamd_rqt_graph_captures(rqamd_rqt* h, int64_t* captures) {
    if (!h || !captures) return rq_fail(RQAMD_ERR_INVALID, "rqt_graph_captures: null argument");
    *captures = h->n_capture;
    return RQAMD_OK;
}

extern "C" int rqamd_rqt_logits(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch,
                                const float* const* codebooks, float* logits_out, void* stream) {
    if (!h || !codes || !codebooks || !logits_out) return rq_fail(RQAMD_ERR_INVALID, "rqt_logits: null argument");
    if (batch < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_logits: batch < 1");
    StepCtx c{};
    c.B = batch; c.codebooks = codebooks; c.temperature = 1.f; c.sample = false; c.logits_out = logits_out;
    return run_all(h, c, codes, cond, 0, false, nullptr, (hipStream_t)stream);
}

extern "C" int rqamd_rqt_forward(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch,
                                 const float* const* codebooks, float* logits_out, float* cond_logits_out, void* stream) {
    if (!h || !codes || !codebooks || !logits_out) return rq_fail(RQAMD_ERR_INVALID, "rqt_forward: null argument");
    if (batch < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_forward: batch < 1");
    if (cond_logits_out && h->cond_len <= 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_forward: cond_logits need block_size_cond > 1");
    StepCtx c{};
    c.B = batch; c.codebooks = codebooks; c.temperature = 1.f; c.sample = false; c.logits_out = logits_out; c.cond_logits_out = cond_logits_out;
    return run_all(h, c, codes, cond, 0, false, nullptr, (hipStream_t)stream);
}

// -------------------------------------------------------------------------------------------------
// One-pass teacher-forced forward: RQTransformer.forward (transformers.py:113-188) the way the reference computes it -- every code is
// known, so the body stack runs ONCE over (image, token) rows and the head stack once over (image, position, depth) rows, instead of
// 64 cached steps that each stream the whole weight set.  Same kernels and arithmetic as the stepped path (run_block's GEMMs and
// resid_ln; embeddings, attention and classifier as position_body / position_depth form them), so the two differ by GEMM tile choice
// only.  Work is chunked by rows: a chunk of images whose body rows fit fwd_chunk_rows, and inside it head sub-chunks of whole
// positions within the same budget; the head rows' order IS the order of the logits, so the classifier writes into logits_out.
// logp form: the classifier writes sub-chunks of rows into a workspace buffer of ~48 MB that log_prob_kernel reduces to one number
// per row -- (B,H,W,D,V) never exists.  No KV cache is read, written or allocated, and h->ws / h->kv are not touched.
// soft_loss form (rqamd_rqt_soft_loss): the same sub-chunks reduced to the soft-target cross entropy of each row, against the caller's
// soft targets (soft_targets) or against softmax(-distance(residual, codebook) / temp) formed per sub-chunk from z (the features the codes
// were quantised from): residual rows, one split-mode quantiser launch into a second buffer of the sub-chunk's size, soft_ce_pair_kernel.
struct OnePassOut {
    float* logits;       // (B,HW,D,V) or null
    float* cond_logits;  // (B, cond_len-1, vocab_size_cond) or null
    float* logp;         // (B,HW,D) or null
    float* cond_logp;    // (B, cond_len-1) or null
    float* soft_loss;    // (B,HW,D) or null
    const float* soft_targets;          // (B,HW,D,V), or
    const float* z;                     // (B,HW,Din) with code_norms[d] (V) and inv_temp
    const float* const* code_norms;
    float inv_temp;
};

int rq_launch_neg_distances(const float* x, const float* codebook, const float* code_norms, int n_embed, long n_vec, int dim, float inv_temp,
                            float* logit_out, float* part_v, int* part_i, hipStream_t st);      // quantize.hip

// the workspace pointers run_block works on, swapped for the duration of a one-pass call (restored on every exit path)
struct WorkspaceSwap {
    rqamd_rqt* h;
    float *x, *xh, *slabs;
    bf16_t *y, *qkv, *ya, *hbuf, *ain;
    explicit WorkspaceSwap(rqamd_rqt* h_) : h(h_), x(h_->x), xh(h_->xh), slabs(h_->slabs), y(h_->y), qkv(h_->qkv), ya(h_->ya), hbuf(h_->hbuf), ain(h_->ain) {}
    ~WorkspaceSwap() { h->x = x; h->xh = xh; h->slabs = slabs; h->y = y; h->qkv = qkv; h->ya = ya; h->hbuf = hbuf; h->ain = ain; }
};

// One-pass prefix prefill ("prefix.one_pass", rqamd_rqt_step_prefill): the codes of spatial positions 0 .. n0-1 of the B rows in h->xs are
// given, so their body tokens need not be stepped.  Tokens 0 .. Pn-1 of every image, Pn = cond_len - 1 + n0 -- all cond_len conditioning
// tokens, then the embeddings of positions 0 .. n0-2 -- run through the body stack in ONE pass the way the reference's first cached step
// does (transformers.py:235-239), and K / V are appended to the layers' caches at 0 .. Pn-1; the device position counter is left at
// n0, where the position loop goes on with the embedding of position n0-1 as its input.  For a text-conditioned model this IS the
// prefill of the text prefix (begin_batch skips its own): one sequence per image, text tokens then code tokens.
// Rows live in h->fws (WorkspaceSwap), chunked over images so that n_img * Pn <= fwd_chunk_rows (one image at least): h->ws / h->kv stay
// where the captured graphs expect them.  Inputs as forward_onepass forms them (gather_codes / body_input with n0 positions per
// image), attention through the appending form of rq_launch_attn_prefill, whichever kernel it picks for Pn tokens: plain up to 255, tiled
// beyond, the one-wavefront-per-token kernel for head sizes other than 64, quantising for the 8-bit caches (Tbody <= 256 there, so Pn <= 255).
static int prefix_prefill(rqamd_rqt* h, const float* const* codebooks, int B, int n0, hipStream_t st) {
    const int E = h->E, D = h->D, HW = h->HW, Pn = h->cond_len - 1 + n0;
    const int vc = h->cfg.vocab_size_cond < 1 ? 1 : h->cfg.vocab_size_cond;
    if (n0 < 1 || n0 >= HW || B < 1 || B > h->cap) return rq_fail(RQAMD_ERR_INVALID, "rqt prefix prefill: %d positions, %d rows (capacity %d)", n0, B, h->cap);
    int n_img = h->fwd_chunk_rows / Pn;            // images per chunk
    if (n_img < 1) n_img = 1;
    if (n_img > B) n_img = B;
    const size_t rows = (size_t)n_img * Pn;        // (h->xh holds the n_img * (n0 - 1) input_mlp rows: fewer)
    const size_t total = 2 * al(rows * E * 4) + al((size_t)h->max_slabs * rows * E * 4) + 2 * al(rows * E * 2) + al(rows * 3 * E * 2)
                         + al(rows * 4 * E * 2) + al(rows * h->Din * 2);
    RQ_TRY(h->fws.reserve(total));
    WorkspaceSwap keep(h);
    char* p = (char*)h->fws.p;
    auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return (void*)r; };
    h->x = (float*)take(rows * E * 4); h->xh = (float*)take(rows * E * 4);
    h->slabs = (float*)take((size_t)h->max_slabs * rows * E * 4);
    h->y = (bf16_t*)take(rows * E * 2); h->ya = (bf16_t*)take(rows * E * 2);
    h->qkv = (bf16_t*)take(rows * 3 * E * 2); h->hbuf = (bf16_t*)take(rows * 4 * E * 2);
    h->ain = (bf16_t*)take(rows * h->Din * 2);
    for (int b0 = 0; b0 < B; b0 += n_img) {
        const int n = B - b0 < n_img ? B - b0 : n_img;
        const int64_t* ccodes = h->xs + (long)b0 * HW * D;
        BodyInputArgs bi{};
        bi.cond = h->cond + (long)b0 * h->cond_len; bi.cond_stride = h->cond_len; bi.cond_len = h->cond_len; bi.vocab_cond = vc;
        bi.cond_emb = h->cond_emb; bi.pos_cond = h->pos_cond; bi.bias_tab = h->body_in_bias; bi.pos_tab = h->pos_hw;
        bi.n_img = n; bi.HW = HW; bi.n_pos = n0; bi.D = D; bi.E = E; bi.x = h->x;
        if (h->in_vq) {
            if (n0 > 1) {
                GatherCodesArgs g{};
                g.codes = ccodes; g.head = 0; g.cumsum = 1; g.row0 = 0; g.rows = n * (n0 - 1); g.HW = HW; g.n_pos = n0; g.D = D; g.dim = h->Din; g.out = h->ain;
                for (int d = 0; d < D; ++d) { g.cb[d] = codebooks[d]; g.K[d] = h->Vd[d]; }
                RQ_TRY(rq_launch_gather_codes(g, st));
                RQ_TRY(step_gemm(h, h->ain, h->Din, h->w_in, g.rows, E, h->Din, EPI_F32, nullptr, nullptr, 0, h->xh, E, nullptr, st));
            }
            bi.emb = h->xh;
        } else {
            bi.codes = ccodes; bi.table = h->tok_emb;
            for (int d = 0; d < D; ++d) { bi.offs[d] = h->tok_offs[d]; bi.V[d] = h->Vd[d]; }
        }
        RQ_TRY(rq_launch_body_input(bi, st));
        Pending pend{nullptr, 0, nullptr};         // (the last layer's fc2 output feeds nothing: no head runs for a prefix position)
        const PrefillCtx pf{b0, n, Pn};
        h->cur_gelu_v2 = h->cfg.gelu_v2 == 1 || h->cfg.gelu_v2 == 3;
        for (auto& L : h->body) RQ_TRY(run_block(h, L, h->x, h->x, pend, nullptr, n * Pn, nullptr, 0, 0, h->Tbody, st, &pf));
    }
    return rq_launch_set_int(h->st, n0, st);
}

// One-pass fill of a kept run ("masked.run_prefill", rqamd_rqt_step_run): no head runs at spatial positions p0 .. p1-1 (1 <= p0 < p1 < HW)
// of the B rows in h->xs, so their body tokens need not be stepped.  The R = p1 - p0 tokens of every row -- the inputs of positions
// p0 .. p1-1, i.e. the embeddings of the codes at p0-1 .. p1-2 with their positional entries; position p0-1 was drawn or kept earlier on
// the same stream -- run through all body layers at once, and every layer appends K / V at cache rows T0 .. T0+R-1, T0 = cond_len - 1 + p0,
// behind the rows the earlier positions wrote (rq_launch_attn_extend).  The device position counter is left at p1.
// Built like prefix_prefill: rows in h->fws (WorkspaceSwap), chunked over images so that n_img * R <= fwd_chunk_rows (one image at
// least); h->ws / h->kv stay where the captured graphs expect them.  Guided and composed calls pass all their (2 + K) Bs rows: no
// conditioning token is among a run's inputs, every block's rows attend over the cache rows its own conditioning wrote.
static int run_prefill(rqamd_rqt* h, const float* const* codebooks, int B, int p0, int p1, hipStream_t st) {
    const int E = h->E, D = h->D, HW = h->HW, R = p1 - p0, T0 = h->cond_len - 1 + p0;
    if (p0 < 1 || R < 1 || p1 > HW || B < 1 || B > h->cap) return rq_fail(RQAMD_ERR_INVALID, "rqt run prefill: positions %d .. %d, %d rows (capacity %d)", p0, p1 - 1, B, h->cap);
    if (!run_prefill_ok(h)) return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt run prefill: head size 64 and a bf16 / fp16 cache needed");
    int n_img = h->fwd_chunk_rows / R;             // images per chunk
    if (n_img < 1) n_img = 1;
    if (n_img > B) n_img = B;
    const size_t rows = (size_t)n_img * R;
    const size_t total = 2 * al(rows * E * 4) + al((size_t)h->max_slabs * rows * E * 4) + 2 * al(rows * E * 2) + al(rows * 3 * E * 2)
                         + al(rows * 4 * E * 2) + al(rows * h->Din * 2);
    RQ_TRY(h->fws.reserve(total));
    WorkspaceSwap keep(h);
    char* p = (char*)h->fws.p;
    auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return (void*)r; };
    h->x = (float*)take(rows * E * 4); h->xh = (float*)take(rows * E * 4);
    h->slabs = (float*)take((size_t)h->max_slabs * rows * E * 4);
    h->y = (bf16_t*)take(rows * E * 2); h->ya = (bf16_t*)take(rows * E * 2);
    h->qkv = (bf16_t*)take(rows * 3 * E * 2); h->hbuf = (bf16_t*)take(rows * 4 * E * 2);
    h->ain = (bf16_t*)take(rows * h->Din * 2);
    for (int b0 = 0; b0 < B; b0 += n_img) {
        const int n = B - b0 < n_img ? B - b0 : n_img;
        const int64_t* ccodes = h->xs + (long)b0 * HW * D;
        BodyInputArgs bi{};
        bi.bias_tab = h->body_in_bias; bi.pos_tab = h->pos_hw; bi.cond_len = h->cond_len;
        bi.n_img = n; bi.HW = HW; bi.run_len = R; bi.q0 = p0; bi.D = D; bi.E = E; bi.x = h->x;
        if (h->in_vq) {
            GatherCodesArgs g{};
            g.codes = ccodes; g.head = 0; g.cumsum = 1; g.row0 = 0; g.rows = n * R; g.HW = HW; g.n_pos = R + 1; g.q0 = p0 - 1; g.D = D; g.dim = h->Din; g.out = h->ain;
            for (int d = 0; d < D; ++d) { g.cb[d] = codebooks[d]; g.K[d] = h->Vd[d]; }
            RQ_TRY(rq_launch_gather_codes(g, st));
            RQ_TRY(step_gemm(h, h->ain, h->Din, h->w_in, g.rows, E, h->Din, EPI_F32, nullptr, nullptr, 0, h->xh, E, nullptr, st));
            bi.emb = h->xh;
        } else {
            bi.codes = ccodes; bi.table = h->tok_emb;
            for (int d = 0; d < D; ++d) { bi.offs[d] = h->tok_offs[d]; bi.V[d] = h->Vd[d]; }
        }
        RQ_TRY(rq_launch_body_input(bi, st));
        Pending pend{nullptr, 0, nullptr};         // (the last layer's fc2 output feeds nothing: no head runs at a position of the run)
        PrefillCtx pf{b0, n, R};
        pf.T0 = T0;
        h->cur_gelu_v2 = h->cfg.gelu_v2 == 1 || h->cfg.gelu_v2 == 3;
        for (auto& L : h->body) RQ_TRY(run_block(h, L, h->x, h->x, pend, nullptr, n * R, nullptr, 0, 0, h->Tbody, st, &pf));
    }
    return rq_launch_set_int(h->st, p1, st);
}

static int forward_onepass(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int B, const float* const* codebooks,
                           const OnePassOut& o, hipStream_t st) {
    h->step_on = false;                            // ends a stepping sequence like any other call
    RQ_TRY(finalize_tables(h, st));
    const int E = h->E, V = h->V, D = h->D, HW = h->HW, Tb = h->Tbody, P = h->cond_len - 1;
    const int vc = h->cfg.vocab_size_cond < 1 ? 1 : h->cfg.vocab_size_cond;
    const bool want_cond = o.cond_logits || o.cond_logp;
    if (want_cond && (!h->w_ccls || h->n_ccls_seen < 4)) return rq_fail(RQAMD_ERR_STATE, "rqt: cond_classifier parameters not set");
    // chunk geometry
    if (Tb > h->fwd_chunk_rows) return rq_fail(RQAMD_ERR_INVALID, "rqt one-pass forward: fwd.chunk_rows = %d holds no image (%d body tokens)", h->fwd_chunk_rows, Tb);
    int n_img = h->fwd_chunk_rows / Tb;            // images per body chunk
    if (n_img < 1) n_img = 1;
    if (n_img > B) n_img = B;
    long n_grp = h->fwd_chunk_rows / D;            // (image, position) groups per head sub-chunk
    if (n_grp < 1) n_grp = 1;
    if (n_grp > (long)n_img * HW) n_grp = (long)n_img * HW;
    const size_t rb = (size_t)n_img * Tb, rh = (size_t)n_grp * D, rows = rb > rh ? rb : rh;
    // logits sub-chunk of the logp / soft_loss forms: fwd_logits_bytes (~48 MB) of fp32 rows, whole depth groups (BatchLinear runs one GEMM per depth over it)
    long cls_grp = (long)((size_t)h->fwd_logits_bytes / ((size_t)V * 4)) / D;
    if (cls_grp < 1) cls_grp = 1;
    if (cls_grp > n_grp) cls_grp = n_grp;
    long ccls_rows = (long)((size_t)h->fwd_logits_bytes / ((size_t)vc * 4));
    if (ccls_rows < 1) ccls_rows = 1;
    if (ccls_rows > (long)n_img * (P > 0 ? P : 1)) ccls_rows = (long)n_img * (P > 0 ? P : 1);
    size_t lg_bytes = 0;
    if (o.logp || o.soft_loss) lg_bytes = (size_t)cls_grp * D * V * 4;
    if (o.cond_logp && (size_t)ccls_rows * vc * 4 > lg_bytes) lg_bytes = (size_t)ccls_rows * vc * 4;
    const size_t total_fwd = al(rb * E * 4) + al(rows * E * 4) + al((size_t)h->max_slabs * rows * E * 4) + 2 * al(rows * E * 2) + al(rows * 3 * E * 2)
                         + al(rows * 4 * E * 2) + al(rows * h->Din * 2) + al(lg_bytes);
    // soft_loss from z: target logits, residual rows and the quantiser's partial minima of one logits sub-chunk (cls_grp * D rows)
    const size_t sub_rows = (size_t)cls_grp * D;
    const size_t tl_bytes = o.z ? sub_rows * V * 4 : 0, rs_bytes = o.z ? sub_rows * h->Din * 4 : 0, pm_bytes = o.z ? sub_rows * 64 * 4 : 0;
    const size_t total = total_fwd + al(tl_bytes) + al(rs_bytes) + 2 * al(pm_bytes);
    RQ_TRY(h->fws.reserve(total));
    WorkspaceSwap keep(h);
    char* p = (char*)h->fws.p;
    auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return (void*)r; };
    h->x = (float*)take(rb * E * 4); h->xh = (float*)take(rows * E * 4);
    h->slabs = (float*)take((size_t)h->max_slabs * rows * E * 4);
    h->y = (bf16_t*)take(rows * E * 2); h->ya = (bf16_t*)take(rows * E * 2);
    h->qkv = (bf16_t*)take(rows * 3 * E * 2); h->hbuf = (bf16_t*)take(rows * 4 * E * 2);
    h->ain = (bf16_t*)take(rows * h->Din * 2);
    float* lg = (float*)take(lg_bytes);
    float* tl = (float*)take(tl_bytes);
    float* rs = (float*)take(rs_bytes);
    float* pm_v = (float*)take(pm_bytes);
    int* pm_i = (int*)take(pm_bytes);
    bool one_cb = true;                            // a shared codebook: one quantiser launch over the rows of all depths
    for (int d = 1; o.z && d < D; ++d) one_cb = one_cb && codebooks[d] == codebooks[0] && o.code_norms[d] == o.code_norms[0];

    for (int b0 = 0; b0 < B; b0 += n_img) {
        const int n = B - b0 < n_img ? B - b0 : n_img;
        const int64_t* ccodes = codes + (long)b0 * HW * D;
        const int64_t* ccond = cond ? cond + (long)b0 * h->cond_len : nullptr;
        const int brows = n * Tb;
        // ---- body input: conditioning tokens + the embeddings of spatial positions 0 .. HW-2 (transformers.py:127-137)
        BodyInputArgs bi{};
        bi.cond = ccond; bi.cond_stride = h->cond_len; bi.cond_len = h->cond_len; bi.vocab_cond = vc; bi.cond_emb = h->cond_emb; bi.pos_cond = h->pos_cond;
        bi.bias_tab = h->body_in_bias; bi.pos_tab = h->pos_hw; bi.n_img = n; bi.HW = HW; bi.n_pos = HW; bi.D = D; bi.E = E; bi.x = h->x;
        if (h->in_vq) {
            if (HW > 1) {
                GatherCodesArgs g{};
                g.codes = ccodes; g.head = 0; g.cumsum = 1; g.row0 = 0; g.rows = n * (HW - 1); g.HW = HW; g.n_pos = HW; g.D = D; g.dim = h->Din; g.out = h->ain;
                for (int d = 0; d < D; ++d) { g.cb[d] = codebooks[d]; g.K[d] = h->Vd[d]; }
                RQ_TRY(rq_launch_gather_codes(g, st));
                RQ_TRY(step_gemm(h, h->ain, h->Din, h->w_in, g.rows, E, h->Din, EPI_F32, nullptr, nullptr, 0, h->xh, E, nullptr, st));
            }
            bi.emb = h->xh;
        } else {
            bi.codes = ccodes; bi.table = h->tok_emb;
            for (int d = 0; d < D; ++d) { bi.offs[d] = h->tok_offs[d]; bi.V[d] = h->Vd[d]; }
        }
        RQ_TRY(rq_launch_body_input(bi, st));
        // ---- body stack over (image, token) rows
        Pending pend{nullptr, 0, nullptr};
        const OnePassCtx bctx{n, Tb, false};
        h->cur_gelu_v2 = h->cfg.gelu_v2 == 1 || h->cfg.gelu_v2 == 3;
        for (auto& L : h->body) RQ_TRY(run_block(h, L, h->x, h->x, pend, nullptr, brows, nullptr, 0, 0, Tb, st, nullptr, &bctx));
        if (pend.slabs || pend.bias) {             // the last fc2's partials (+ bias) into the stream: both heads read it row by row
            ResidLnArgs r{};
            r.x_in = h->x; r.x_out = h->x; r.slabs = pend.slabs; r.n_slabs = pend.n; r.bias = pend.bias; r.rows = brows; r.E = E; r.eps = 1e-5f;
            RQ_TRY(rq_launch_resid_ln(r, st));
        }
        // ---- cond_classifier over the body outputs of tokens 0 .. cond_len-2 (transformers.py:150-153)
        if (want_cond && P > 0) {
            for (long r0 = 0; r0 < (long)n * P; r0 += ccls_rows) {
                const int nr = (int)((long)n * P - r0 < ccls_rows ? (long)n * P - r0 : ccls_rows);
                HeadInputArgs hi{};                // (rows (image, t < P) of the stream, gathered: "depth 0" rows of groups of one, nothing added)
                hi.xbody = h->x; hi.Tb = Tb; hi.tok0 = 0; hi.HW = P; hi.D = 1; hi.E = E; hi.row0 = r0; hi.rows = nr; hi.xh = h->xh; hi.pos_d = nullptr;
                RQ_TRY(rq_launch_head_input(hi, st));
                ResidLnArgs r{};
                r.x_in = h->xh; r.gamma = h->ccls_lnw; r.beta = h->ccls_lnb; r.y = h->y; r.rows = nr; r.E = E; r.eps = 1e-5f;
                RQ_TRY(rq_launch_resid_ln(r, st));
                float* dst = o.cond_logits ? o.cond_logits + ((long)b0 * P + r0) * vc : lg;
                RQ_TRY(step_gemm(h, h->y, E, h->w_ccls, nr, vc, E, EPI_F32, h->b_ccls, nullptr, 0, dst, vc, nullptr, st));
                if (o.cond_logp) {                 // log p(cond[t + 1] | cond[: t + 1])
                    if (!cond) return rq_fail(RQAMD_ERR_INVALID, "rqt_log_probs: cond_logp_out without cond");
                    LogProbArgs lp{};
                    lp.logits = dst; lp.ld = vc; lp.rows = nr; lp.V = vc; lp.targets = ccond; lp.row0 = r0; lp.t_per = P; lp.t_stride = h->cond_len; lp.t_off = 1;
                    lp.out = o.cond_logp + (long)b0 * P + r0;
                    RQ_TRY(rq_launch_log_prob(lp, st));
                }
            }
        }
        // ---- head stack over (image, position, depth) rows, sub-chunks of whole positions
        const long groups = (long)n * HW;
        for (long g0 = 0; g0 < groups; g0 += n_grp) {
            const long ng = groups - g0 < n_grp ? groups - g0 : n_grp;
            const int hrows = (int)(ng * D);
            HeadInputArgs hi{};
            hi.xbody = h->x; hi.Tb = Tb; hi.tok0 = h->cond_len - 1; hi.bias_tab = h->head_in_bias; hi.pos_d = h->pos_d;
            hi.row0 = g0 * D; hi.rows = hrows; hi.HW = HW; hi.D = D; hi.E = E; hi.xh = h->xh;
            if (h->head_vq) {
                if (D > 1) {
                    GatherCodesArgs g{};
                    g.codes = ccodes; g.head = 1; g.cumsum = h->cumsum ? 1 : 0; g.row0 = g0 * D; g.rows = hrows; g.HW = HW; g.D = D; g.dim = h->Din; g.out = h->ain;
                    for (int d = 0; d < D; ++d) { g.cb[d] = codebooks[d]; g.K[d] = h->Vd[d]; }
                    RQ_TRY(rq_launch_gather_codes(g, st));
                        RQ_TRY(step_gemm(h, h->ain, h->Din, h->w_headin, hrows, E, h->Din, EPI_F32, nullptr, nullptr, 0, h->xh, E, nullptr, st));
                }
            } else {
                hi.codes = ccodes; hi.table = h->tok_emb;
                for (int d = 0; d < D; ++d) { hi.offs[d] = h->tok_offs[d]; hi.V[d] = h->Vd[d]; }
            }
            RQ_TRY(rq_launch_head_input(hi, st));
            Pending hp{nullptr, 0, nullptr};
            const OnePassCtx hctx{(int)ng, D, true};
            h->cur_gelu_v2 = h->cfg.gelu_v2 == 1 || h->cfg.gelu_v2 == 2;
            for (auto& L : h->head) RQ_TRY(run_block(h, L, h->xh, h->xh, hp, nullptr, hrows, nullptr, 0, 0, D, st, nullptr, &hctx));
            ResidLnArgs r{};
            r.x_in = h->xh; r.slabs = hp.slabs; r.n_slabs = hp.n; r.bias = hp.bias;
            r.gamma = h->cls_lnw; r.beta = h->cls_lnb; r.y = h->y; r.rows = hrows; r.E = E; r.eps = 1e-5f;
            RQ_TRY(rq_launch_resid_ln(r, st));
            // classifier: the shared matrix over all rows, or BatchLinear's matrix of each depth over that depth's rows (stride D).
            // Teacher-forced logits are not LogitMask-ed (see position_depth).
            const long row_g = ((long)b0 * HW + g0) * D;       // first row of this sub-chunk in the outputs
            const long step_g = o.logits ? ng : cls_grp;
            for (long c0 = 0; c0 < ng; c0 += step_g) {
                const long cg = ng - c0 < step_g ? ng - c0 : step_g;
                float* dst = o.logits ? o.logits + (row_g + c0 * D) * V : lg;
                const bf16_t* A = h->y + c0 * D * E;
                if (h->shared_cls) {
                    RQ_TRY(step_gemm(h, A, E, h->w_cls, (int)(cg * D), V, E, EPI_F32, h->b_cls, nullptr, 0, dst, V, nullptr, st));
                } else {
                    for (int d = 0; d < D; ++d)
                        RQ_TRY(step_gemm(h, A + (long)d * E, D * E, h->w_cls + (long)d * V * E, (int)cg, V, E, EPI_F32, h->b_cls + (long)d * V, nullptr, 0,
                                         dst + (long)d * V, D * V, nullptr, st));
                }
                if (o.logp) {
                    LogProbArgs lp{};
                    lp.logits = dst; lp.ld = V; lp.rows = (int)(cg * D); lp.V = V; lp.targets = codes; lp.row0 = row_g + c0 * D; lp.t_per = 1; lp.t_stride = 1; lp.t_off = 0;
                    lp.out = o.logp + row_g + c0 * D;
                    RQ_TRY(rq_launch_log_prob(lp, st));
                }
                if (o.soft_loss) {
                    SoftCeArgs sc{};
                    sc.logits = dst; sc.ld = V; sc.rows = (int)(cg * D); sc.V = V; sc.out = o.soft_loss + row_g + c0 * D;
                    if (o.soft_targets) {
                        sc.targets = o.soft_targets + (row_g + c0 * D) * V; sc.ldt = V;
                    } else {
                        ResidRowsArgs rr{};
                        rr.z = o.z; rr.codes = codes; rr.vec0 = (long)b0 * HW + g0 + c0; rr.n_vec = cg; rr.D = D; rr.dim = h->Din; rr.out = rs;
                        for (int d = 0; d < D; ++d) { rr.cb[d] = codebooks[d]; rr.K[d] = V; }
                        RQ_TRY(rq_launch_resid_rows(rr, st));
                        if (one_cb) {
                            RQ_TRY(rq_launch_neg_distances(rs, codebooks[0], o.code_norms[0], V, cg * D, h->Din, o.inv_temp, tl, pm_v, pm_i, st));
                        } else {
                            for (int d = 0; d < D; ++d)
                                RQ_TRY(rq_launch_neg_distances(rs + (size_t)d * cg * h->Din, codebooks[d], o.code_norms[d], V, cg, h->Din, o.inv_temp,
                                                               tl + (size_t)d * cg * V, pm_v, pm_i, st));
                        }
                        sc.targets = tl; sc.ldt = V; sc.pair_D = D; sc.pair_nv = cg;
                    }
                    RQ_TRY(rq_launch_soft_ce(sc, st));
                }
            }
        }
    }
    return RQAMD_OK;
}

extern "C" int rqamd_rqt_forward_onepass(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch,
                                         const float* const* codebooks, float* logits_out, float* cond_logits_out, void* stream) {
    if (!h || !codes || !codebooks || !logits_out) return rq_fail(RQAMD_ERR_INVALID, "rqt_forward_onepass: null argument");
    if (batch < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_forward_onepass: batch < 1");
    if (cond_logits_out && h->cond_len <= 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_forward_onepass: cond_logits need block_size_cond > 1");
    if (h->seen.size() - h->n_ccls_seen < h->n_required)
        return rq_fail(RQAMD_ERR_STATE, "rqt: only %zu of %zu parameters set", h->seen.size() - h->n_ccls_seen, h->n_required);
    OnePassOut o{};
    o.logits = logits_out; o.cond_logits = cond_logits_out;
    return forward_onepass(h, codes, cond, batch, codebooks, o, (hipStream_t)stream);
}

extern "C" int rqamd_rqt_log_probs(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch,
                                   const float* const* codebooks, float* logp_out, float* cond_logp_out, void* stream) {
    if (!h || !codes || !codebooks || !logp_out) return rq_fail(RQAMD_ERR_INVALID, "rqt_log_probs: null argument");
    if (batch < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_log_probs: batch < 1");
    if (cond_logp_out && h->cond_len <= 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_log_probs: cond_logp needs block_size_cond > 1");
    if (cond_logp_out && !cond) return rq_fail(RQAMD_ERR_INVALID, "rqt_log_probs: cond_logp_out without cond");
    if (h->seen.size() - h->n_ccls_seen < h->n_required)
        return rq_fail(RQAMD_ERR_STATE, "rqt: only %zu of %zu parameters set", h->seen.size() - h->n_ccls_seen, h->n_required);
    OnePassOut o{};
    o.logp = logp_out; o.cond_logp = cond_logp_out;
    return forward_onepass(h, codes, cond, batch, codebooks, o, (hipStream_t)stream);
}

// rqamd_rqt_soft_loss (include/rqamd.h): the soft-target cross entropy of every code under the same pass
extern "C" int rqamd_rqt_soft_loss(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch, const float* const* codebooks,
                                   const float* soft_targets, const float* z, const float* const* code_norms, float temp, float* loss_out,
                                   float* cond_logp_out, void* stream) {
    if (!h || !codes || !codebooks || !loss_out) return rq_fail(RQAMD_ERR_INVALID, "rqt_soft_loss: null argument");
    if (batch < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_soft_loss: batch < 1");
    if ((soft_targets != nullptr) == (z != nullptr)) return rq_fail(RQAMD_ERR_INVALID, "rqt_soft_loss: exactly one of soft_targets and z must be given");
    if (cond_logp_out && h->cond_len <= 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_soft_loss: cond_logp needs block_size_cond > 1");
    if (cond_logp_out && !cond) return rq_fail(RQAMD_ERR_INVALID, "rqt_soft_loss: cond_logp_out without cond");
    for (int d = 0; d < h->D; ++d)
        if (h->Vd[d] != h->V)
            return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_soft_loss: vocab_sizes[%d] = %d != %d: one vocabulary for all depths needed (the soft codes are concatenated along depth)",
                           d, h->Vd[d], h->V);
    OnePassOut o{};
    o.soft_loss = loss_out; o.cond_logp = cond_logp_out; o.soft_targets = soft_targets;
    if (z) {
        if (!code_norms) return rq_fail(RQAMD_ERR_INVALID, "rqt_soft_loss: z without code_norms");
        for (int d = 0; d < h->D; ++d)
            if (!codebooks[d] || !code_norms[d]) return rq_fail(RQAMD_ERR_INVALID, "rqt_soft_loss: null codebook / code_norms[%d]", d);
        if (!(temp > 0.f)) return rq_fail(RQAMD_ERR_INVALID, "rqt_soft_loss: temp must be > 0");
        if (h->Din % 64 != 0 || h->Din < 64 || h->Din > 256)
            return rq_fail(RQAMD_ERR_UNSUPPORTED, "rqt_soft_loss: input_embed_dim %d must be 64, 128, 192 or 256 to form the targets from z", h->Din);
        o.z = z; o.code_norms = code_norms; o.inv_temp = 1.0f / temp;
    }
    if (h->seen.size() - h->n_ccls_seen < h->n_required)
        return rq_fail(RQAMD_ERR_STATE, "rqt: only %zu of %zu parameters set", h->seen.size() - h->n_ccls_seen, h->n_required);
    return forward_onepass(h, codes, cond, batch, codebooks, o, (hipStream_t)stream);
}

// ---- lanes (round 6): a second handle that runs on the SAME parameter arena as `src` -- its own workspace, KV caches, graphs and
// stepping state, no weights of its own.  Two handles fed half a batch each on two streams run two independent decode chains
// over one copy of the weights (L2 / MALL hits for whichever chain reaches a layer second).
extern "C" int rqamd_dbg_rqt_share_params(rqamd_rqt* dst, const rqamd_rqt* src) {
    if (!dst || !src) return rq_fail(RQAMD_ERR_INVALID, "rqt_share_params: null argument");
    if (memcmp(&dst->cfg, &src->cfg, sizeof(dst->cfg)) != 0 || (!dst->head.empty() && dst->head[0].nh != src->head[0].nh))
        return rq_fail(RQAMD_ERR_INVALID, "rqt_share_params: configurations differ");
    if (src->seen.size() - src->n_ccls_seen < src->n_required || src->tables_dirty)
        return rq_fail(RQAMD_ERR_STATE, "rqt_share_params: the source handle has not run yet (parameters incomplete or tables not derived)");
    auto cp = [](std::vector<RqtLayer>& d, const std::vector<RqtLayer>& s) {
        for (size_t i = 0; i < d.size(); ++i) {
            RqtLayer keep = d[i];
            d[i] = s[i];
            d[i].kc = keep.kc; d[i].vc = keep.vc; d[i].ksc = keep.ksc; d[i].vsc = keep.vsc; d[i].kcs = keep.kcs; d[i].vcs = keep.vcs;
        }
    };
    cp(dst->body, src->body); cp(dst->head, src->head);
    dst->w_in = src->w_in; dst->w_headin = src->w_headin; dst->w_cls = src->w_cls;
    dst->b_in = src->b_in; dst->b_headin = src->b_headin; dst->b_cls = src->b_cls; dst->cls_lnw = src->cls_lnw; dst->cls_lnb = src->cls_lnb;
    dst->w_ccls = src->w_ccls; dst->b_ccls = src->b_ccls; dst->ccls_lnw = src->ccls_lnw; dst->ccls_lnb = src->ccls_lnb; dst->n_ccls_seen = src->n_ccls_seen;
    dst->cond_emb = src->cond_emb; dst->pos_cond = src->pos_cond; dst->pos_hw = src->pos_hw; dst->pos_d = src->pos_d; dst->tok_emb = src->tok_emb;
    dst->body_in_bias = src->body_in_bias; dst->head_in_bias = src->head_in_bias;
    dst->seen = src->seen; dst->tables_dirty = false; dst->gvalid = false;
    dst->arena.release();
    return RQAMD_OK;
}

// ---- stepping form: the caller draws the samples (include/rqamd.h)
extern "C" int rqamd_rqt_step_begin(rqamd_rqt* h, const int64_t* partial, const int64_t* cond, int batch, const float* const* codebooks, void* stream) {
    if (!h || !partial || !codebooks) return rq_fail(RQAMD_ERR_INVALID, "rqt_step_begin: null argument");
    if (batch < 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_step_begin: batch < 1");
    h->step_on = false;
    for (int d = 0; d < h->D; ++d) h->step_cb[d] = codebooks[d];
    StepCtx c{};
    c.B = batch; c.codebooks = h->step_cb; c.temperature = 1.f; c.sample = false;
    RQ_TRY(begin_batch(h, c, partial, cond, (hipStream_t)stream));
    h->step_on = true; h->step_B = batch; h->step_pos = 0; h->step_d = 0;
    return RQAMD_OK;
}

// the body-only steps (p, -1), p < n_pos, of a sequence that has just begun, in one pass (prefix_prefill; whatever "prefix.one_pass" says).
// The text prefix that step_begin has cached is run again as the head of the merged sequences: the same rows, rewritten
extern "C" int rqamd_rqt_step_prefill(rqamd_rqt* h, int n_pos, void* stream) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "rqt_step_prefill: null handle");
    if (!h->step_on || h->step_pos != 0 || h->step_d != 0)
        return rq_fail(RQAMD_ERR_STATE, "rqt_step_prefill: valid only directly after rqamd_rqt_step_begin");
    if (n_pos < 1 || n_pos > h->HW - 1) return rq_fail(RQAMD_ERR_INVALID, "rqt_step_prefill: n_pos = %d outside 1 .. %d", n_pos, h->HW - 1);
    if (h->cap < h->step_B) return rq_fail(RQAMD_ERR_STATE, "rqt_step_prefill: the workspace was re-sized by another call");
    RQ_TRY(prefix_prefill(h, h->step_cb, h->step_B, n_pos, (hipStream_t)stream));
    h->step_pos = n_pos; h->step_d = 0;
    return RQAMD_OK;
}

// the body-only steps (p, -1), p0 <= p < p1, of a sequence that stands at position p0 >= 1, in one pass (run_prefill; whatever
// "masked.run_prefill" says).  A handle run_prefill does not serve (8-bit cache, another head size) takes the steps themselves
extern "C" int rqamd_rqt_step_run(rqamd_rqt* h, int p0, int p1, void* stream) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "rqt_step_run: null handle");
    if (!h->step_on) return rq_fail(RQAMD_ERR_STATE, "rqt_step_run: no rqamd_rqt_step_begin");
    if (p0 < 1 || p1 <= p0 || p1 > h->HW - 1)
        return rq_fail(RQAMD_ERR_INVALID, "rqt_step_run: positions p0 = %d .. p1 = %d outside 1 <= p0 < p1 <= %d", p0, p1, h->HW - 1);
    if (h->step_pos != p0 || h->step_d != 0)
        return rq_fail(RQAMD_ERR_STATE, "rqt_step_run: the sequence stands at step (%d, %d), not at position %d with no head step taken", h->step_pos, h->step_d, p0);
    if (h->cap < h->step_B) return rq_fail(RQAMD_ERR_STATE, "rqt_step_run: the workspace was re-sized by another call");
    hipStream_t st = (hipStream_t)stream;
    if (run_prefill_ok(h)) {
        RQ_TRY(run_prefill(h, h->step_cb, h->step_B, p0, p1, st));
    } else {
        StepCtx c{};
        c.B = h->step_B; c.codebooks = h->step_cb; c.temperature = 1.f; c.sample = false;
        for (int pos = p0; pos < p1; ++pos) {
            RQ_TRY(rq_launch_set_int(h->st, pos, st));
            Pending pend;
            RQ_TRY(position_body(h, c, false, pos, pend, st));
        }
    }
    h->step_pos = p1; h->step_d = 0;
    return RQAMD_OK;
}

extern "C" int rqamd_rqt_step_logits(rqamd_rqt* h, int pos, int d, const float** logits_dev, void* stream) {
    if (!h || !h->step_on) return rq_fail(RQAMD_ERR_STATE, "rqt_step_logits: no rqamd_rqt_step_begin");
    const bool body_only = d < 0;
    if (pos != h->step_pos || (body_only ? h->step_d != 0 : d != h->step_d) || pos >= h->HW)
        return rq_fail(RQAMD_ERR_INVALID, "rqt_step_logits: step (%d, %d) out of order, expected (%d, %d)", pos, d, h->step_pos, h->step_d);
    if (h->cap < h->step_B) return rq_fail(RQAMD_ERR_STATE, "rqt_step_logits: the workspace was re-sized by another call");
    hipStream_t st = (hipStream_t)stream;
    StepCtx c{};
    c.B = h->step_B; c.codebooks = h->step_cb; c.temperature = 1.f; c.sample = false;
    if (body_only || d == 0) {
        RQ_TRY(rq_launch_set_int(h->st, pos, st));
        Pending pend;
        RQ_TRY(position_body(h, c, pos == 0, pos, pend, st));
        h->step_pend_slabs = pend.slabs; h->step_pend_n = pend.n; h->step_pend_bias = pend.bias;
    }
    if (body_only) { h->step_pos = pos + 1; h->step_d = 0; return RQAMD_OK; }
    if (!logits_dev) return rq_fail(RQAMD_ERR_INVALID, "rqt_step_logits: null argument");
    const Pending pend{h->step_pend_slabs, h->step_pend_n, h->step_pend_bias};
    RQ_TRY(position_depth(h, c, d, pend, pos, true, st));
    *logits_dev = h->logits;
    if (d + 1 < h->D) h->step_d = d + 1;
    else { h->step_d = 0; h->step_pos = pos + 1; }
    return RQAMD_OK;
}

__global__ void set_codes_kernel(int64_t* xs, const int64_t* codes, int rows, long stride, int slot) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) xs[(long)r * stride + slot] = codes[r];
}

extern "C" int rqamd_rqt_step_set_code(rqamd_rqt* h, int pos, int d, const int64_t* codes, void* stream) {
    if (!h || !h->step_on || !codes) return rq_fail(RQAMD_ERR_STATE, "rqt_step_set_code: no step in progress / null argument");
    if (pos < 0 || pos >= h->HW || d < 0 || d >= h->D) return rq_fail(RQAMD_ERR_INVALID, "rqt_step_set_code: step (%d, %d)", pos, d);
    RQ_LAUNCH(set_codes_kernel, dim3((unsigned)((h->step_B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->xs, codes, h->step_B,
              (long)h->HW * h->D, pos * h->D + d);
    return rq_check_launch("set_codes_kernel");
}

extern "C" int rqamd_rqt_step_end(rqamd_rqt* h, int64_t* codes_out, void* stream) {
    if (!h || !h->step_on) return rq_fail(RQAMD_ERR_STATE, "rqt_step_end: no step in progress");
    h->step_on = false;
    if (codes_out) RQ_HIP(hipMemcpyAsync(codes_out, h->xs, (size_t)h->step_B * h->HW * h->D * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RQAMD_OK;
}

extern "C" int rqamd_rqt_set_profile(rqamd_rqt* h, int profile) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "null handle");
    h->prof.on = profile == 1;
    if (h->prof.skip_gemm != (profile == 2)) h->gvalid = false;      // the captured graphs hold (or lack) the GEMM nodes
    h->prof.skip_gemm = profile == 2;
    return RQAMD_OK;
}
extern "C" int rqamd_rqt_get_profile_attn(rqamd_rqt* h, double* ms, int64_t* launches) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "null handle");
    if (ms) *ms = h->prof.attn_ms_total;
    if (launches) *launches = h->prof.attn_launches;
    return RQAMD_OK;
}
extern "C" int rqamd_rqt_get_profile(rqamd_rqt* h, double* ms, int64_t* launches, double* bytes, double* flops) {
    if (!h) return rq_fail(RQAMD_ERR_INVALID, "null handle");
    if (ms) *ms = h->prof.ms_total;
    if (launches) *launches = h->prof.launches;
    if (bytes) *bytes = h->prof.bytes;
    if (flops) *flops = h->prof.flops;
    return RQAMD_OK;
}
