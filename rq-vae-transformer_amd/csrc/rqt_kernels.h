// rqt_kernels.h -- non-GEMM kernels of the RQ-Transformer decode step (gfx950).
//
// Reference call sites (rqvae/models/rqtransformer/):
//   resid_ln_kernel     <- x + attn / x + mlp residual adds and nn.LayerNorm (attentions.py:126-142,
//                          transformers.py:91); also reduces the split-K partial slabs of the
//                          producing GEMM (launch-boundary reduce) and adds its bias
//   attn_decode_kernel  <- MultiSelfAttention.forward with caching=True (attentions.py:60-104):
//                          KV append (torch.cat :75-76), q.(k^T/sqrt(hs)) :87, causal mask :88-91,
//                          softmax :92, att.v :95 -- one wavefront per (batch row, head)
//   embed_tokens_kernel <- model_aux.get_code_emb_with_depth + .sum(-2) / cumsum(-2)
//                          (transformers.py:109-111,218-225,249-257), only for the NEW position
//   cond_embed_kernel   <- cond_emb(cond) + pos_emb_cond (transformers.py:224)
//   sample_kernel       <- sample_from_logits (rqvae/utils/utils.py:82-123), no host sync
//   one-pass forward    <- RQTransformer.forward (transformers.py:113-188) over all positions at once: gather_codes_kernel /
//                          body_input_kernel / head_input_kernel (the inputs of the two stacks, :127-137,:160-175), attn_prefill_kernel
//                          without a cache (body), attn_packed_kernel (depth groups of the head stack), log_prob_kernel
//                          (F.cross_entropy's log_softmax + gather, :371-381, one number per logits row)
#pragma once
#include "rq_hip.h"

struct ResidLnArgs {
    const float* x_in;      // [rows][E]
    float* x_out;           // [rows][E] (may alias x_in); may be null when only y is wanted
    const float* slabs;     // [n_slabs][rows][E] split-K partials of the producing GEMM, or null
    int n_slabs;
    const float* bias;      // [E] bias of the producing GEMM, or null
    const float* addvec;    // [E] broadcast add (positional embedding), or null
    const float* gamma;     // LayerNorm weight/bias; null => no LN output
    const float* beta;
    bf16_t* y;              // [rows][E] bf16 LN output
    int rows, E;
    float eps;
};

struct AttnDecodeArgs {
    const bf16_t* qkv;      // [rows][3E]: q | k | v, head h at columns h*hd..h*hd+hd-1 of each third (hd = E / nh; 64 in every released config)
    bf16_t* kc;             // K cache [rows][nh][Tcap][hd]
    bf16_t* vc;             // V cache [rows][nh][Tcap][hd]
    float* ksc;             // null: bf16 keys.  Non-null (opt-in RQAMD_KV=int8k, body stack): `kc` holds [rows][nh][Tcap][64] BYTES,
                            // key component = (byte - 128) * ksc[row][head][position], one absmax / 127 scale per cached key
    float* vsc;             // null: bf16 values.  Non-null (opt-in RQAMD_KV=int8kv; needs ksc): `vc` holds bytes + these scales, like the keys
    bf16_t* y;              // [rows][E]
    const int* step;        // device-side step counter (or null)
    int step_off;           // t = *step + step_off = number of cached keys before this token
    int t_max;              // host-side upper bound of t for this launch (selects the register-block count), -1 = Tcap-1
    int rows, nh, E, Tcap;
};

// Decode attention of a shared-prompt sampling call (rqt_attn_shared.hip): the `fan` consecutive rows of a group share one copy of the
// conditioning prefix.  Global key j < Ps is row j of the group's cache, key j >= Ps is row j - Ps of the row's own cache; this token
// (global index t >= Ps) is appended at own row t - Ps.  Head size 64, bf16 / fp16, Ps + Tcap <= 256.
struct AttnSharedArgs {
    const bf16_t* qkv;      // [rows][3E], as AttnDecodeArgs
    const bf16_t* kcs;      // group K cache [rows / fan][nh][Ps][64], read only
    const bf16_t* vcs;      // group V cache, likewise
    bf16_t* kc;             // own K cache [rows][nh][Tcap][64]
    bf16_t* vc;             // own V cache
    bf16_t* y;              // [rows][E]
    const int* step;        // device-side step counter (or null)
    int step_off;           // t = *step + step_off = global index of this token's key
    int t_max;              // host-side upper bound of t (selects the register-block count), -1 = Ps + Tcap - 1
    int rows, fan, nh, E, Ps, Tcap;
};
int rq_launch_attn_shared(const AttnSharedArgs& a, hipStream_t s);

// Multi-token prefill of the conditioning prefix (transformers.py:235-239 of the reference: the first cached body step
// runs the whole prefix through MultiSelfAttention.forward with the causal mask, attentions.py:60-104).
struct AttnPrefillArgs {
    const bf16_t* qkv;      // [n_img * P][3E], row = img * P + i (token i of image img)
    bf16_t* kc;             // K cache of the FIRST image of this chunk: [n_img][nh][Tcap][64]; positions 0..P-1 are written.  Null (with vc, ksc,
                            // vsc): the cache-free form of the one-pass teacher-forced forward -- nothing is appended anywhere
    bf16_t* vc;
    float* ksc;             // as AttnDecodeArgs::ksc (of the first image of the chunk), or null
    float* vsc;             // as AttnDecodeArgs::vsc, or null
    bf16_t* y;              // [n_img * P][E]
    int n_img, P, nh, E, Tcap;
};

// Multi-token causal attention that extends a cache which already holds rows 0 .. T0-1 (rqt_attn_extend.hip; the one-pass fill of an
// interior kept run, engine_rqt.hip: run_prefill): query r of the R new tokens attends over the cached rows and the run's own keys
// 0 .. r, token r is appended at cache row T0 + r.  Head size 64, bf16 / fp16, T0 + R <= Tcap <= RQAMD_RQT_MAX_CONTEXT.  Bit for bit the
// rows R of the prefill kernels over T0 + R tokens.
struct AttnExtendArgs {
    const bf16_t* qkv;      // [n_img * R][3E], row = img * R + r
    bf16_t* kc;             // K cache of the FIRST image of this chunk: [n_img][nh][Tcap][64]; rows < T0 are read, rows T0 .. T0+R-1 written
    bf16_t* vc;
    bf16_t* y;              // [n_img * R][E]
    int n_img, R, T0, nh, E, Tcap;
};
int rq_launch_attn_extend(const AttnExtendArgs& a, hipStream_t s);

struct EmbedTokArgs {
    const int64_t* xs;      // [rows][HW][D] codes
    const float* cb[8];     // per-depth codebooks (K, dim), padding row excluded
    int K[8];
    const int* pos;         // device-side spatial position
    int pos_off;            // position read = *pos + pos_off
    int depth_lo;           // sum over depths [depth_lo, n_depth) (0: the depth cumsum; n_depth - 1: cumsum_depth_ctx off)
    int n_depth;
    int rows, HW, D, dim;
    bf16_t* out;            // [rows][dim]
};

struct SampleArgs {
    const float* logits;    // [rows][V]
    int rows, V;
    float temperature;
    int top_k;              // <=0 or >=V: off
    float top_p;            // <0: off
    const uint64_t* rng;    // device {seed, offset}; or null -> seed/offset below
    uint64_t seed, offset;
    const int* pos;         // device-side spatial position (or null)
    int d, D;               // depth index / depth count: draw counter = offset + (*pos * D + d)
    int64_t* out;           // samples: out[row * out_stride + (*pos * D + d)] (pos null -> out[row*out_stride])
    long out_stride;
    float* probs_out;       // [rows][V] filtered distribution, or null
    int* redo;              // [rows] workspace: rows the top-k kernel hands to the general kernel (null: general kernel only)
    const uint8_t* keep;    // keep[row * keep_stride + (*pos * D + d)] != 0: the code is given -- no draw, `out` and `redo` untouched (null: draw every row)
    long keep_stride;
    // classifier-free guidance (rqamd_rqt_sample_guided): row `row` is drawn from guide(logits[row], logits_u[row], gscale), mixed where
    // the kernel loads the row -- no guided-logits buffer exists
    const float* logits_u;  // [rows][V] logits of the unconditional twins, or null: unguided
    float gscale;           // guidance scale s: g = c + (s - 1) (c - u)
    long out_mirror;        // != 0: the drawn code is also written to out[(row * out_stride + slot) + out_mirror] (the twin's slot); 0: none
    // per-row parameters (rqamd_sample_logits_rows / rqamd_rqt_sample_rows): row_temperature non-null selects the per-row kernels
    // (rqt_sample_rows.hip), which read the scalars above from these device arrays instead -- row r is drawn exactly as a scalar call with
    // r's values draws it.  row_top_k / row_top_p are read at [row * D + d] and are required with row_temperature.
    const float* row_temperature;   // [rows], or null: the scalar kernels
    const int* row_top_k;           // [rows * D]
    const float* row_top_p;         // [rows * D]
    const float* row_gscale;        // [rows], or null: gscale above for every row
    const uint64_t* row_seeds;      // [rows], or null: rng / seed above.  Non-null: row r draws with key row_seeds[r], Philox row field 0
                                    // and counter offset + slot (rng is ignored) -- the stream of row 0 of a call seeded with row_seeds[r]
    // log-probability of the draw (rqamd_sample_logits_logp / rqamd_rqt_sample_logp): non-null selects the LOGP instantiations
    // (rqt_sample_logp.hip), which also write log(probability of the drawn code in the distribution the draw was made from) to
    // logp_out[row * out_stride + slot] -- addressed like `out`, no mirror; kept codes write nothing.  Same codes as with null.
    float* logp_out;
    // min-p and locally typical sampling (rqamd_sample_logits_trunc / rqamd_rqt_sample_trunc): a row with either filter on takes the
    // TRUNC instantiations (rqt_sample_trunc.hip), which run the two stages after top-p, each on the renormalised output of the stage
    // before it.  Off values (the defaults here) and null tables: the kernels above, bit for bit.  The tables are read at
    // [row * D + d] like row_top_p and need row_temperature; a null table leaves the scalar in force for every row.
    float min_p = 0.f;              // <= 0: off; else drop q_i < min_p * max q
    float typical_p = -1.f;         // < 0 or >= 1: off; else the prefix of the |surprisal - entropy| order that reaches this mass
    const float* row_min_p = nullptr;       // [rows * D], or null
    const float* row_typical_p = nullptr;   // [rows * D], or null
    // sampling schedules over positions and depths (rqamd_rqt_sample_schedule): sched != 0 selects the SCHED instantiations of the
    // per-row kernels (rqt_sample_sched.hip), which read EVERY table above -- row_temperature and row_gscale included, row_seeds not --
    // at [row * row_stride + *pos * D + d]: row_stride = HW * D for a schedule per image, 0 for one shared by all rows.  `pos` is
    // required.  Row r at (pos, d) is drawn exactly as the per-row kernels draw it with the values the tables hold there.
    int sched = 0;
    // composed guidance (rqamd_rqt_sample_compose: K extra row blocks behind the twins): the drawn code also goes to
    // out[(row * out_stride + slot) + j * out_mirror] for j = 2 .. 1 + out_mirror_n.  0: the one twin of out_mirror alone, as before
    int out_mirror_n = 0;
    long row_stride = 0;
};

// Classifier-free guidance: the logit a guided row is drawn from, u + s (c - u) written as c + (s - 1)(c - u) so that s = 1 returns c
// bit for bit; a masked column (LogitMask: -inf in both rows) stays -inf instead of becoming inf - inf.  Raw logits, before the
// temperature.  THE one place logits are mixed: the three samplers call it where they load their row, guide_logits_kernel for the
// host paths.
static __device__ __forceinline__ float guide_logit(float c, float u, float s) {
    return c == -__int_as_float(0x7f800000) ? c : fmaf(s - 1.0f, c - u, c);
}

// Composed guidance (rqamd_rqt_sample_compose, rqamd_compose_logits): K <= RQ_MAX_EXTRA_CONDS extra conditionings with raw logits x_k and
// weights w_k next to the pair (c, u).  The target is G = u + s (c - u) + sum_k w_k (x_k - u).  The extra term is folded into BOTH rows of
// the pair, in fp32 and in this order,
//     e = 0;  for k = 0 .. K-1:  e = fmaf(w_k, x_k - u, e)
//     (c == -inf || e == 0) ?  c' = c, u' = u  :  c' = c + e, u' = u + e
// and the samplers then draw from guide_logit(c', u', s) as they draw any guided pair: c' - u' is c - u up to rounding, so that is G.
// Two rules are part of the contract.  c == -inf: LogitMask leaves -inf in the same columns of every row, x_k - u is inf - inf there and
// e is NaN -- the pair stays as it is and guide_logit returns -inf.  e == 0 (every weight zero, every extra row equal to u): the pair
// stays bit for bit -- c + 0.0f would turn a -0.0 logit into +0.0, which the samplers' order keys tell apart.
// THE one place extra conditions enter: the fold kernel of the engine and rqamd_compose_logits call it (rqt_compose.hip).
enum { RQ_MAX_EXTRA_CONDS = 4 };
static __device__ __forceinline__ void compose_pair(float c, float u, const float (&x)[RQ_MAX_EXTRA_CONDS], const float (&w)[RQ_MAX_EXTRA_CONDS],
                                                    int K, float& c_out, float& u_out) {
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < RQ_MAX_EXTRA_CONDS; ++k)
        if (k < K) e = fmaf(w[k], x[k] - u, e);
    const bool same = c == -__int_as_float(0x7f800000) || e == 0.f;
    c_out = same ? c : c + e;
    u_out = same ? u : u + e;
}

// The fold of composed guidance (rqt_compose.hip).  Row r of the pair: c[r], u[r]; extra k: x[(k * rows + r)][:]; weights w[k * rows + r].
// out_u non-null (the engine's fold): c' -> out_c[r], u' -> out_u[r].  out_u null (rqamd_compose_logits): guide_logit(c', u', scale) -> out_c[r].
struct ComposeArgs {
    const float *c, *u;     // [rows][V] each
    const float* x;         // [K][rows][V]
    const float* w;         // [K][rows], device
    int rows, V, K;
    float* out_c;           // [rows][V]
    float* out_u;           // [rows][V] or null
    float scale;
};
int rq_launch_compose(const ComposeArgs& a, hipStream_t s);

// Anchored sampling (rqamd_rqt_sample_anchor, rqamd_anchor_logits): the logit of code v gets the quantiser's soft-code term of the residual
// the anchored image has at this depth, x' = x - w * dist(r, codebook[v]), dist the fp32 squared distance of rq_launch_neg_distances.
// Three rules are part of the contract.  l == -inf: LogitMask columns stay -inf.  w == 0: the logit stays bit for bit (fmaf(-0, dist, l)
// would turn a -0.0 logit into +0.0, which the samplers' order keys tell apart).  A distance that is not finite -- NaN, or the +inf the
// expanded form gives where an infinite component of z meets a code component of the other sign; a finite z row never has one -- leaves
// the logit alone, so an image with a non-finite z row degrades to unanchored instead of to an all -inf row.
// THE one place the anchor enters: the fold kernel of the engine and rqamd_anchor_logits call it (rqt_anchor.hip).
static __device__ __forceinline__ float anchor_logit(float l, float dist, float w) {
    const float inf = __int_as_float(0x7f800000);
    return (l == -inf || w == 0.f || !(fabsf(dist) < inf)) ? l : fmaf(-w, dist, l);
}

// r[b][:] = z[b * z_stride + p * dim ..] - cb[0][c_0] - ... - cb[d-1][c_{d-1}], c_j = codes[b * code_stride + p * code_D + j], p = pos ? *pos : 0,
// subtracted one depth after the other in fp32 as the quantiser does (resid_rows_kernel): stateless, recomputed from z at every depth.
// Only codes of depths < d are read.  A code outside 0 .. K-1 traps, as rq_embed_kernel does.
struct AnchorResidArgs {
    const float* z;
    long z_stride;          // floats between the rows of two images (engine: HW * dim; rows given one by one: dim)
    const int64_t* codes;
    long code_stride;       // codes between two images (engine: HW * D; rows given one by one: d)
    int code_D;             // codes per position (engine: D)
    const int* pos;         // device position counter, or null (position 0)
    const float* cb[8];
    int K;                  // codes per codebook
    int d, dim, rows;       // dim % 4 == 0
    float* out;             // [rows][dim]
};
int rq_launch_anchor_resid(const AnchorResidArgs& a, hipStream_t s);

// out_c[r][v] = anchor_logit(c[r][v], dist[r][v], w_r), and with u non-null out_u[r][v] = anchor_logit(u[r][v], dist[r][v], w_r): the twins of a
// guided pair get the same term, so guide_logit(c', u', s) is the guided mix minus w * dist up to rounding.
// w_r = w[r * w_row_stride + (pos ? *pos : 0) * D + d], a workgroup-uniform load.
struct AnchorFoldArgs {
    const float *c, *u;     // [rows][V]; u null: unguided
    const float* dist;      // [rows][V]
    const float* w;         // device
    long w_row_stride;      // 0: one table for all rows
    const int* pos;         // device position counter, or null
    int D, d;
    int rows, V;
    float *out_c, *out_u;   // [rows][V]; out_u with u
};
int rq_launch_anchor_fold(const AnchorFoldArgs& a, hipStream_t s);
// the three stages of one anchored step over `rows` rows: residual -> resid, distances -> dist (part_v / part_i: rows * 64 each), fold
int rq_launch_anchor_step(const AnchorResidArgs& r, const float* codebook, const float* code_norms, float* dist, float* part_v, int* part_i,
                          const AnchorFoldArgs& f, hipStream_t s);

int rq_launch_sample_sched(const SampleArgs& a, hipStream_t s);     // rqt_sample_sched.hip
// is a filter of the TRUNC instantiations in effect (scalars), or could one be (tables)?
static inline bool rq_sample_trunc_on(const SampleArgs& a) {
    return a.row_min_p || a.row_typical_p || a.min_p > 0.f || (a.typical_p >= 0.f && a.typical_p < 1.0f);
}
int rq_launch_sample_trunc(const SampleArgs& a, hipStream_t s);     // rqt_sample_trunc.hip

int rq_launch_guide_logits(const float* c, const float* u, int rows, int V, float scale, float* out, hipStream_t s);
int rq_launch_resid_ln(const ResidLnArgs& a, hipStream_t s);
int rq_launch_attn_decode(const AttnDecodeArgs& a, hipStream_t s);
int rq_launch_attn_prefill(const AttnPrefillArgs& a, hipStream_t s);
int rq_launch_embed_tokens(const EmbedTokArgs& a, hipStream_t s);
// x[(img, i)] = cond_emb[cond[img][i]] + pos_emb_cond[i] for i < n_tok: the prefix rows of the prefill
int rq_launch_cond_embed_multi(const int64_t* cond, int cond_stride, int n_tok, const float* cond_emb, int vocab_cond,
                               const float* pos_emb_cond, float* x, int n_img, int E, hipStream_t s);
int rq_launch_cond_embed(const int64_t* cond, int cond_stride, int cond_idx, const float* cond_emb, int vocab_cond,
                         const float* pos_emb_cond, float* x, int rows, int E, hipStream_t s);
int rq_launch_sample(const SampleArgs& a, hipStream_t s);
// learned token embeddings (tok_emb: nn.Embedding, or TupleEmbedding = per-depth tables at row offsets offs[d], primitives.py:25-75):
// x[b][:] = sum_{d in [d_lo, d_hi)} table[offs[d] + code[b][pos][d]][:] + add[row][:], row = (pos_dev ? *pos_dev : 0) + add_row
struct TokEmbedArgs {
    const int64_t* xs;      // [rows][HW][D] codes
    const float* table;     // [sum V][E] fp32
    int offs[8], V[8];
    const int* pos;         // device-side spatial position (or null)
    int pos_off;            // code position = *pos + pos_off
    int d_lo, d_hi;
    const float* add;       // [*][E] positional table
    int add_by_pos;         // 1: row = *pos + add_row, 0: row = add_row
    int add_row;
    int rows, HW, D, E;
    float* out;             // [rows][E] fp32
};
int rq_launch_tok_embed(const TokEmbedArgs& a, hipStream_t s);
// logits[:, v_lo:V] = -inf (per-depth vocabularies smaller than the classifier's width)
int rq_launch_mask_logits(float* logits, int rows, int V, int v_lo, hipStream_t s);
int rq_launch_cvt_bf16(const float* src, bf16_t* dst, long n, hipStream_t s);
// dst[c][r] = bf16(src[r][c]): BatchLinear's (in, out) matrices into the GEMM's K-contiguous weight layout
int rq_launch_cvt_bf16_transpose(const float* src, bf16_t* dst, int R, int Cc, hipStream_t s);
// ---- one-pass teacher-forced forward (engine_rqt.hip: forward_onepass): every position of a chunk of images at once.
// Body rows are ordered (image, token), head rows (image, position, depth) -- the order of the logits.

// codebook rows summed over depth -> bf16 GEMM operand, for all rows of a chunk (embed_tokens_kernel for one position at a time):
//   body (head == 0): row R = (image, q), q = 0 .. n_pos-2: sum over all depths of the codes at spatial position q.  n_pos = HW: every
//        position that is ever embedded (the one-pass forward); n_pos = n0 < HW: the given prefix of a sampling call (engine_rqt.hip:
//        prefix_prefill), whose position n0-1 the first decode step embeds.  HW stays the stride of `codes`
//   head (head == 1): row R = (g, d), g = image * HW + position: sum over depths [cumsum ? 0 : d-1, d) of the codes at g (d == 0: zeros)
struct GatherCodesArgs {
    const int64_t* codes;   // [n_img][HW][D] codes of the chunk
    const float* cb[8];     // per-depth codebooks (K, dim), padding row excluded
    int K[8];
    int head, cumsum;
    long row0;              // first row of this launch (rows are counted from the start of the chunk)
    int rows, HW, D, dim;
    int n_pos;              // body form: positions per image, n_pos - 1 rows each (2 .. HW); the head form ignores it
    int q0;                 // body form: the first code position of every image, rows q = q0 .. q0 + n_pos - 2 (0 everywhere but in the run form
                            // of engine_rqt.hip: run_prefill; q0 + n_pos <= HW)
    bf16_t* out;            // [rows][dim]
};
int rq_launch_gather_codes(const GatherCodesArgs& a, hipStream_t s);

// body input rows (image, t), t = 0 .. Tb-1, Tb = cond_len - 1 + n_pos (n_pos = HW: the whole map; n_pos = n0: a given prefix): t < cond_len: cond_emb[cond[image][t]] + pos_emb_cond[t]; else, with q = t - cond_len:
// emb[(image, q)] + bias_tab[q] (emb = the input_mlp GEMM over GatherCodesArgs rows), or -- table non-null -- pos_tab[q] + sum_d table[offs[d] + code_d]
struct BodyInputArgs {
    const int64_t* cond;    // [n_img][cond_stride] or null (class 0)
    int cond_stride, cond_len, vocab_cond;
    const float *cond_emb, *pos_cond;
    const float* emb;       // [n_img * (n_pos-1)][E] or null
    const float* bias_tab;  // [HW][E] (body_in_bias)
    const int64_t* codes;   // [n_img][HW][D] (learned token embeddings only)
    const float* table;     // [sum V][E] or null
    int offs[8], V[8];
    const float* pos_tab;   // [HW][E] (pos_emb_hw)
    int n_img, HW, D, E;
    int n_pos;              // positions per image, 1 .. HW (HW is the stride of `codes` and the height of the tables)
    int run_len, q0;        // run form (run_len > 0; engine_rqt.hip: run_prefill): rows (image, r), r = 0 .. run_len-1, are the inputs of positions
                            // q0 + r (q0 >= 1): the embedding of the codes at q0 - 1 + r, emb [n_img * run_len][E]; cond and n_pos are unused.  0: the forms above
    float* x;               // [n_img * Tb][E]
};
int rq_launch_body_input(const BodyInputArgs& a, hipStream_t s);

// head input rows (g, d): d == 0: body output of token cond_len-1 + position of the image + pos_emb_d[0]; d >= 1: xh (holding the
// head_mlp GEMM over GatherCodesArgs rows) += bias_tab[d], or -- table non-null -- pos_d[d] + table[offs[d-1] + code_{d-1}]
struct HeadInputArgs {
    const float* xbody;     // [n_img * Tb][E]
    int Tb, tok0;           // tok0 = cond_len - 1
    const float* bias_tab;  // [D][E] (head_in_bias)
    const float* pos_d;     // [D][E]; null with D == 1: a plain gather of rows tok0 .. tok0 + HW - 1 of every image (cond_classifier input)
    const int64_t* codes;   // [n_img][HW][D] (learned token embeddings only)
    const float* table;
    int offs[8], V[8];
    long row0;
    int rows, HW, D, E;
    float* xh;              // [rows][E]
};
int rq_launch_head_input(const HeadInputArgs& a, hipStream_t s);

// causal attention inside groups of `group` <= 8 consecutive rows (the depth axis of the head stack): one lane per (row, head), the
// group's keys / values straight from the qkv rows; same arithmetic as the decode kernels
struct AttnPackedArgs {
    const bf16_t* qkv;      // [rows][3E]
    bf16_t* y;              // [rows][E]
    int rows, group, nh, E; // rows % group == 0
};
int rq_launch_attn_packed(const AttnPackedArgs& a, hipStream_t s);

// out[r] = logits[r][target] - logsumexp(logits[r][:]) in fp32; target = targets[(R / t_per) * t_stride + R % t_per + t_off], R = row0 + r
// (NaN where the target is outside 0 .. V-1)
struct LogProbArgs {
    const float* logits;    // [rows][ld]
    long ld;
    int rows, V;
    const int64_t* targets;
    long row0;
    int t_per, t_stride, t_off;
    float* out;             // [rows]
    // step form (pos non-null): target = targets[R * t_stride + slot] and the result goes to out[R * t_stride + slot], slot =
    // *pos * slot_D + slot_d -- one launch of a sampling step, over all its rows, after the sampler has written the code
    const int* pos;
    int slot_D, slot_d;
};
int rq_launch_log_prob(const LogProbArgs& a, hipStream_t s);

// Soft-target cross entropy of logits rows (rqvae/optimizer/loss.py:68-76): out[r] = sum_v -t_v (x_v - m - log(sum exp(x - m) + 1e-7)),
// m = max_v x_v, fp32.  Plain form (pair_D == 0): t = targets[r][:], any non-negative weights.  Pair form (pair_D > 0): `targets` holds
// target LOGITS a, t = softmax(a) formed in the same pass; the rows of the two matrices pair up as logits row r = (g, d) of
// pair_D depths <-> target row d * pair_nv + g (the depth-major order the residual rows and the quantiser launches use).
struct SoftCeArgs {
    const float* logits;    // [rows][ld]
    long ld;
    const float* targets;   // [rows][ldt]
    long ldt;
    int rows, V;
    int pair_D;
    long pair_nv;
    float* out;             // [rows]
};
int rq_launch_soft_ce(const SoftCeArgs& a, hipStream_t s);

// residual rows of given codes: out[d * n_vec + g][:] = z[vec0 + g][:] - e_0(c_0) - ... - e_{d-1}(c_{d-1}), c = codes[vec0 + g][:], subtracted
// one depth after the other in fp32 as the quantiser does (csrc/quantize.hip: rq_split_combine_kernel), so the rows carry its bits
struct ResidRowsArgs {
    const float* z;         // [.][dim]
    const int64_t* codes;   // [.][D]
    const float* cb[8];
    int K[8];
    long vec0, n_vec;
    int D, dim;             // dim % 4 == 0
    float* out;             // [D][n_vec][dim]
};
int rq_launch_resid_rows(const ResidRowsArgs& a, hipStream_t s);

int rq_launch_set_int(int* p, int v, hipStream_t s);
int rq_launch_add_int(int* p, int v, hipStream_t s);
