/* rqamd.h -- C ABI of librqamd.so: the MI355X (gfx950) RQ-VAE + RQ-Transformer sampling path.
 *
 * The reference (kakaobrain/rq-vae-transformer) is pure Python on PyTorch and has no FFI or
 * operator registry; its "operator API" for this path is the Python method surface
 * of rqvae.models.  Each entry point below names the reference method(s) it stands
 * behind (file:line relative to the reference root).  The host-side mirror of those classes lives in
 * rq-vae-transformer_amd/rqvae/ and binds this ABI with ctypes.
 *
 * Conventions
 *  - plain C: device pointers, sizes, an opaque stream (hipStream_t passed as void*; NULL = stream 0).
 *  - every call is asynchronous on `stream` unless stated; the library never frees or keeps caller
 *    buffers beyond the call, except the parameter tables of the engine handles (see *_set_param).
 *  - return 0 on success, negative rqamd_status otherwise; rqamd_last_error() gives the message
 *    (thread-local).  Nothing is thrown across the ABI.
 *  - tensors are dense, row-major, in the layouts the reference methods use.
 *
 * Two builds of the RQ-Transformer engine (round 6).  librqamd.so stores weights, GEMM operands and the KV cache as bfloat16
 * (BASELINE.json's compute dtype; the default everywhere).  librqamd_f16.so is the SAME source compiled with -DRQ_F16=1
 * (csrc/rq_hip.h): IEEE fp16 storage instead, fp32 accumulation / residual stream / LayerNorm / softmax / logits as before --
 * what the reference's `amp=True` (fp16 autocast, rqvae/models/rqtransformer/transformers.py:21,206; main_sampling_fid.py:216)
 * computes in.  It exports the rqamd_rqt_* and (since the end of round 6) the rqamd_vae_* entry points below with identical signatures
 * and meaning, plus rqamd_abi_version / rqamd_last_error / rqamd_dbg_set_row_scale; the quantiser (fp32 arithmetic) exists in
 * librqamd.so only.  The fp16 RQ-VAE engine is opt-in on the Python side (RQAMD_VAE=fp16): three more mantissa bits in every stored
 * activation and weight -- z_e and pixels ~8 x closer to the fp32 reference -- for ~5 % more decode time.  Values beyond 65504 become
 * inf in fp16 storage, as in torch.float16.
 */
#ifndef RQAMD_H
#define RQAMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RQAMD_ABI_VERSION 7

typedef enum {
    RQAMD_OK = 0,
    RQAMD_ERR_INVALID = -1,      /* bad argument / shape (reference raises ValueError / AssertionError) */
    RQAMD_ERR_UNSUPPORTED = -2,  /* shape outside what the gfx950 kernels implement */
    RQAMD_ERR_HIP = -3,          /* HIP runtime error */
    RQAMD_ERR_STATE = -4,        /* handle not ready (missing parameters) */
    RQAMD_ERR_NOMEM = -5         /* hipMalloc of an engine workspace ran out of device memory; the handle is left empty (not
                                    dangling) and the call may be retried after the caller released memory */
} rqamd_status;

int rqamd_abi_version(void);
const char* rqamd_last_error(void);

/* ---- residual quantiser -------------------------------------------------------------------
 * rqamd_rq_quantize <- RQBottleneck.quantize (rqvae/models/rqvae/quantizations.py:237-271), i.e.
 * VQEmbedding.compute_distances :43-62 + find_nearest_embedding :64-69 + embed :144-146 fused over
 * all depths.  x (n_vec, dim) fp32; codebooks[d] (n_embed[d], dim) fp32 WITHOUT the padding row
 * (pass weight[:-1]); the same pointer repeated = shared codebook.  codes (n_vec, depth) int64;
 * quant_cum (depth, n_vec, dim) fp32 cumulative quants (quant_list) or NULL.
 * code_norms[d] (n_embed[d]) fp32 = ||c||^2 per code from rqamd_rq_code_norms, owned and cached by the caller per codebook
 * version (no library-side scratch: calls on different streams / threads never share state).
 * Distances use the reference's expanded form ||x||^2+||c||^2-2x.c in fp32; ties -> lowest index.
 * workspace (caller-owned device scratch, n_vec * dim * 4 + n_vec * 64 * 8 bytes, or NULL): lets small inputs (< 96 tiles
 * of 64 vectors: the per-image rFID / get_codes calls) divide the codebook over the chip, one launch pair per depth; the
 * result is bit-identical to the single-launch path. */
int rqamd_rq_quantize(const float* x, const float* const* codebooks, const float* const* code_norms, const int* n_embed,
                      int depth, int64_t n_vec, int dim, int64_t* codes, float* quant_cum, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* rqamd_rq_soft_codes <- RQBottleneck.get_soft_codes (quantizations.py:371-400): per depth, soft_out[v][d][:] =
 * softmax(-distances(residual_d, codebook) / temp) (n_vec, depth, n_embed) fp32 and codes[v][d] = argmin of the distances,
 * or -- stochastic != 0 -- one multinomial draw from that soft code (Philox keyed by seed / offset); the residual is updated
 * with the chosen code.  All codebooks must have one size.  workspace: n_vec * (dim * 4 + 512 + n_embed * 4) bytes. */
int rqamd_rq_soft_codes(const float* x, const float* const* codebooks, const float* const* code_norms, const int* n_embed,
                        int depth, int64_t n_vec, int dim, float temp, int stochastic, uint64_t seed, uint64_t offset,
                        float* soft_out, int64_t* codes, void* workspace, int64_t workspace_bytes, void* stream);
/* rqamd_rq_distances <- VQEmbedding.compute_distances (quantizations.py:43-62) on its own: dist_out[v][k] =
 * ||x_v||^2 + ||c_k||^2 - 2 x_v . c_k  (n_vec, n_embed) fp32, the values the quantiser's argmin and the soft codes are formed
 * from (same kernel, same summation order), for ONE codebook.  workspace: n_vec * 64 * 8 bytes of device scratch.  (ABI v5) */
int rqamd_rq_distances(const float* x, const float* codebook, const float* code_norms, int n_embed, int64_t n_vec, int dim,
                       float* dist_out, void* workspace, int64_t workspace_bytes, void* stream);
/* rqamd_rq_code_norms <- the codebook_t.pow(2).sum(0) term of compute_distances (quantizations.py:51-52). */
int rqamd_rq_code_norms(const float* codebook, int n_embed, int dim, float* norms_out, void* stream);

/* ---- EMA codebook update (stage-1 training; VQEmbedding._update_buffers / _update_embedding, quantizations.py:80-129) ----
 * rqamd_rq_ema_accumulate <- :85-99: count_out[k] = number of vectors whose nearest code is k, sum_out[k][:] = their sum (the
 *   reference's one_hot.sum(1) and one_hot @ vectors), x (n_vec, dim) fp32, idx (n_vec) int64, added in ascending vector order
 *   (deterministic; no (n_embed x n_vec) one-hot matrix).  The caller all-reduces both over the ranks (:101-103) before
 * rqamd_rq_ema_update <- :105-118: cluster_size_ema = decay * cluster_size_ema + (1 - decay) * count, embed_ema likewise with sum;
 *   restart_vectors (n_embed, dim) fp32 or NULL: the dead-code restart with the caller's random vectors (usage = cluster_size_ema
 *   >= 1; unused codes take the random vector and cluster size 1).  In place.  decay is a double (ABI v4): torch computes the step
 *   as mul_(decay) then add_(x, alpha = 1 - decay) with alpha taken in double, and so does the kernel.
 * rqamd_rq_ema_normalize <- :120-129: weight_out[k][:] = embed_ema[k][:] / (n (cluster_size_ema[k] + eps) / (n + n_embed eps)),
 *   n = *n_total, a device scalar holding sum(cluster_size_ema) (computed by the caller). */
int rqamd_rq_ema_accumulate(const float* x, const int64_t* idx, int64_t n_vec, int dim, int n_embed, float* count_out,
                            float* sum_out, void* stream);
int rqamd_rq_ema_update(float* cluster_size_ema, float* embed_ema, const float* count, const float* sum,
                        const float* restart_vectors, int n_embed, int dim, double decay, void* stream);
int rqamd_rq_ema_normalize(const float* cluster_size_ema, const float* embed_ema, const float* n_total, int n_embed, int dim,
                           float eps, float* weight_out, void* stream);

/* rqamd_rq_embed <- RQBottleneck.embed_code :297-311 (mode 0: sum over depth),
 * embed_code_with_depth :313-334 (mode 1: (n_vec, depth, dim)), and the depth-cumsum the sampler
 * feeds to head_mlp (transformers.py:157-160; mode 2).  codes (n_vec, depth) int64; out fp32.
 * code == n_embed selects the zero padding row (quantizations.py:28).  Any other out-of-range code is an index error in
 * the reference (F.embedding's device-side assert); here the kernel traps, which surfaces as a HIP error at the next
 * synchronisation -- it cannot be reported asynchronously through the return value, and it is never silent zeros. */
int rqamd_rq_embed(const int64_t* codes, const float* const* codebooks, const int* n_embed, int depth,
                   int64_t n_vec, int dim, int mode, float* out, void* stream);

/* ---- sampler ------------------------------------------------------------------------------
 * rqamd_sample_logits <- sample_from_logits / top_k_logits / top_p_probs (rqvae/utils/utils.py:60-123):
 * fp32, /temperature, keep logits >= k-th largest (ties kept), NaN -> -inf, softmax, nucleus filter
 * (first token whose inclusive cumulative mass reaches p is kept), renormalise, one multinomial draw
 * per row by the exponential race max_i p_i/E_i (the algorithm torch.multinomial uses for one sample)
 * on Philox4x32-10 keyed by (seed, offset).  No host synchronisation.  top_k <= 0 or >= vocab: no
 * top-k; top_p < 0: no nucleus step (top_p = 1.0 still runs it, as the reference does,
 * transformers.py:323-324).  probs_out (rows, vocab) fp32 receives the filtered distribution
 * (parity hook) or NULL; samples_out (rows) int64 or NULL.  row_flags: caller-owned scratch of `rows` ints (lets rows
 * whose top-k survivors fit in registers skip the general kernel) or NULL. */
int rqamd_sample_logits(const float* logits, int rows, int vocab, float temperature, int top_k,
                        float top_p, uint64_t seed, uint64_t offset, int64_t* samples_out,
                        float* probs_out, int* row_flags, void* stream);
/* rqamd_soft_ce <- soft_target_cross_entropy(reduction='none') (rqvae/optimizer/loss.py:68-84) over `rows` rows (additive, ABI v7):
 * loss_out[r] = sum_v -t_v (x_v - m - log(sum_v exp(x_v - m) + 1e-7)), m = max_v x_v, x = logits[r * ld_logits + v], t = targets[r *
 * ld_targets + v], fp32 throughout.  The targets need not sum to 1; an all-zero row gives 0.  Non-finite logits behave as there: a NaN
 * logit, or -inf under a zero target (0 * -inf), makes the row NaN; -inf under a positive target gives +inf. */
int rqamd_soft_ce(const float* logits, int64_t ld_logits, const float* targets, int64_t ld_targets, int64_t rows, int vocab,
                  float* loss_out, void* stream);
/* rqamd_sample_logits with a temperature, top-k and top-p per row (not in the reference); additive, ABI v7.  temperature, top_k,
 * top_p: DEVICE arrays of `rows` entries; seeds: a device array of `rows` Philox keys, or NULL.  Row r is filtered and drawn exactly
 * as row r of rqamd_sample_logits(logits, rows, vocab, temperature[r], top_k[r], top_p[r], seed, offset, ...) over the same matrix
 * and the same row_flags -- samples_out and probs_out bit for bit, whichever of the three sampler kernels that call would take.
 * With seeds, row r draws with key seeds[r] and Philox row 0 instead: what row 0 of the one-row call
 * rqamd_sample_logits(logits + r * vocab, 1, ..., seeds[r], offset, ...) draws, wherever the row stands in the matrix (seed is
 * then unused).  top_k[r] <= 0 or >= vocab and top_p[r] < 0 mean "off", as above.  Nothing is read on the host and no state is
 * kept: the caller validates temperature > 0 (the kernels trap on no value; a temperature <= 0 or NaN draws an arbitrary code). */
int rqamd_sample_logits_rows(const float* logits, int rows, int vocab, const float* temperature, const int* top_k,
                             const float* top_p, const uint64_t* seeds, uint64_t seed, uint64_t offset,
                             int64_t* samples_out, float* probs_out, int* row_flags, void* stream);
/* The draw and its log-probability (not in the reference); additive, ABI v7.  One entry point for the four forms of the sampler:
 * logits_u NULL: unguided, else row r is drawn from guide(logits[r], logits_u[r], s) as rqamd_rqt_sample_guided draws it, s =
 * guidance_scale or row_gscale[r]; row_temperature NULL: the scalar kernels with temperature / top_k / top_p, else the per-row kernels
 * with the DEVICE arrays row_temperature, row_top_k, row_top_p (both required then), row_gscale and row_seeds (each or NULL), as in
 * rqamd_sample_logits_rows.  samples_out (rows) int64 and draw_logp_out (rows) fp32 are both required: samples_out is bit for bit
 * what the entry point without log-probabilities draws from the same arguments, and draw_logp_out[r] = log of the probability the
 * drawn code had in the distribution row r was drawn from (after guidance, temperature, top-k, top-p and renormalisation; +0.0
 * where one code survives).  row_flags as above. */
int rqamd_sample_logits_logp(const float* logits, const float* logits_u, int rows, int vocab,
                             float temperature, int top_k, float top_p, float guidance_scale,
                             const float* row_temperature, const int* row_top_k, const float* row_top_p,
                             const float* row_gscale, const uint64_t* row_seeds, uint64_t seed, uint64_t offset,
                             int64_t* samples_out, float* draw_logp_out, int* row_flags, void* stream);
/* Min-p and locally typical sampling (not in the reference); additive, ABI v7.  The arguments of rqamd_sample_logits_logp (the four
 * forms of the sampler), two more filters, and probs_out / draw_logp_out each optional (at least one of samples_out and probs_out;
 * draw_logp_out needs samples_out).  Per row, each stage acts on the renormalised output of the stage before it: guidance and
 * temperature, top-k, NaN scrub and softmax, top-p -- all as in rqamd_sample_logits -- then
 *   min-p    (0 < min_p <= 1): drop every code whose probability is below min_p times the largest; the leader always stays;
 *   typical  (0 <= typical_p < 1): over the codes with q > 0, H = -sum q log q and a_i = |-log q_i - H|; the codes in ascending order
 *            of a (ties: lowest vocabulary index first) up to and including the first whose inclusive cumulative mass reaches
 *            typical_p are kept -- the inclusive rule of top-p; typical_p = 0 keeps the first code of that order;
 * then one draw by the exponential race on the Philox counter of rqamd_sample_logits.  min_p <= 0: min-p off; typical_p < 0 or >= 1:
 * typical off.  A non-finite scalar, or min_p > 1, is RQAMD_ERR_INVALID with nothing written.  row_min_p / row_typical_p: DEVICE arrays
 * of `rows` entries with row_temperature, each or NULL (NULL: the scalar for every row); they are not validated, like the other
 * per-row arrays.  A row with both filters off is drawn -- samples_out, probs_out, draw_logp_out, row_flags -- bit for bit as the
 * existing entry points draw it, by the kernel their class rule selects; a row with either on never takes the streaming kernel, and
 * the register kernel hands rows back to the general one exactly where it does today.  probs_out holds the distribution after all
 * stages; draw_logp_out[r] the log of the drawn code's probability in it (+0.0 where one code survives). */
int rqamd_sample_logits_trunc(const float* logits, const float* logits_u, int rows, int vocab,
                              float temperature, int top_k, float top_p, float min_p, float typical_p, float guidance_scale,
                              const float* row_temperature, const int* row_top_k, const float* row_top_p,
                              const float* row_min_p, const float* row_typical_p,
                              const float* row_gscale, const uint64_t* row_seeds, uint64_t seed, uint64_t offset,
                              int64_t* samples_out, float* probs_out, float* draw_logp_out, int* row_flags, void* stream);

/* ---- RQ-VAE encoder / decoder engine -------------------------------------------------------
 * Handle = packed bf16 weights + activation workspace for Encoder/Decoder (modules.py:10-202),
 * quant_conv / post_quant_conv (rqvae.py:68-69).  Parameters are pushed by their reference
 * state_dict names ("decoder.up.3.block.1.conv2.weight", ...), fp32 device pointers in torch layout. */
typedef struct rqamd_vae rqamd_vae;
typedef struct {
    int ch, out_ch, in_channels, resolution, z_channels, num_res_blocks;
    int n_levels;             /* len(ch_mult) */
    int ch_mult[8];
    int n_attn_res;
    int attn_resolutions[8];
    int embed_dim;            /* RQVAE embed_dim (quant_conv out / post_quant_conv in) */
    int double_z;
} rqamd_vae_config;

int rqamd_vae_create(const rqamd_vae_config* cfg, rqamd_vae** out);
int rqamd_vae_destroy(rqamd_vae* h);
/* options of a handle that the config struct does not carry (ABI v7).  "resamp_with_conv" = 0 | 1 <- ddconfig.resamp_with_conv (modules.py:12,103;
 * layers.py:20-57): 1 (default, every released config) = Upsample / Downsample carry their 3 x 3 conv; 0 = bare nearest-2x
 * upsample / 2 x 2 average pool, no `*.upsample.conv.*` / `*.downsample.conv.*` parameters. */
int rqamd_vae_set_option(rqamd_vae* h, const char* name, int value);
/* copies + repacks (fp32 -> bf16, OIHW -> O,kh,kw,I) on `stream`; the source may be freed after
 * the stream reaches this point. */
int rqamd_vae_set_param(rqamd_vae* h, const char* name, const float* dev_ptr, const int64_t* shape,
                        int ndim, void* stream);
/* rqamd_vae_decode <- RQVAE.decode (rqvae.py:85-89) + Decoder.forward (modules.py:171-202):
 * z_q (batch, h, w, embed_dim) fp32 NHWC -> out (batch, out_ch, H, W) fp32 NCHW. */
int rqamd_vae_decode(rqamd_vae* h, const float* z_q, int batch, float* out, void* stream);
/* rqamd_vae_encode <- RQVAE.encode (rqvae.py:80-83) + Encoder.forward (modules.py:73-98):
 * x (batch, in_channels, H, W) fp32 NCHW -> z_e (batch, h, w, embed_dim) fp32 NHWC. */
int rqamd_vae_encode(rqamd_vae* h, const float* x, int batch, float* z_e, void* stream);

/* ---- RQ-Transformer sampling engine --------------------------------------------------------
 * Handle = packed bf16 weights, fixed-capacity KV caches, device-side step state and (optionally)
 * captured hipGraphs for RQTransformer.sample / cached_forward (transformers.py:190-369),
 * AttentionStack/AttentionBlock/MultiSelfAttention (attentions.py:39-169) and the classifier. */
typedef struct rqamd_rqt rqamd_rqt;
typedef struct {
    int embed_dim, n_head;
    int n_layer_body, n_layer_head;
    int vocab_size;           /* shared classifier / codebook size */
    int input_embed_dim;      /* codebook dim fed to input_mlp/head_mlp */
    int vocab_size_cond, block_size_cond;
    int H, W, D;              /* block_size */
    int gelu_v2;              /* attentions.py:25-36: 0 = exact erf GELU ('v1') in both stacks, 1 = x*sigmoid(1.702x) ('v2') in both;
                                 2 = body 'v1' / head 'v2', 3 = body 'v2' / head 'v1' (the stacks have their own block configs) */
    /* stage-2 flags (transformers.py:60-99; every released config sets all five): 0 selects the primitives.py variants --
     * learned token embeddings (nn.Embedding / TupleEmbedding "tok_emb") instead of the RQ-VAE codebook through
     * input_mlp / head_mlp, no depth cumsum in the head context, one classifier matrix per depth (BatchLinear) */
    int input_emb_vqvae, head_emb_vqvae, shared_tok_emb, shared_cls_emb, cumsum_depth_ctx;
    int vocab_sizes[8];       /* per-depth vocabulary (all equal to vocab_size unless shared_* are off); vocab_size = max */
} rqamd_rqt_config;

/* Longest body context, H * W + block_size_cond - 1 tokens: 32 x 32 positions behind 64 text tokens (1087).  Contexts beyond 256 tokens
 * need head size 64 in the body stack and the bf16 / fp16 KV cache (RQAMD_KV unset); rqamd_rqt_create refuses everything else. */
#define RQAMD_RQT_MAX_CONTEXT 1088
int rqamd_rqt_create(const rqamd_rqt_config* cfg, rqamd_rqt** out);
int rqamd_rqt_destroy(rqamd_rqt* h);
/* options of a handle that the config struct does not carry (ABI v7).  "head.n_head" <- head.block.n_head where it differs from
 * body.block.n_head = cfg.n_head (transformers.py:86-87: each AttentionStack has its own block config; attentions.py:44-57: any
 * embed_dim / n_head).  Head size 64 -- every released config -- takes the tuned attention kernels; any other size <= 256 a plain
 * wavefront-per-(row, head) kernel (bf16 / fp16 cache only: the RQAMD_KV 8-bit formats need 64).
 * "prefix.one_pass" (0 | 1, default 0; additive, ABI v7): how rqamd_rqt_sample, _sample_masked, _sample_guided and _sample_rows (armed by
 * rqamd_rqt_sample_logp or not) bring the given leading positions into the body stack's KV cache.  n0 = the number of leading
 * positions before start_h / start_w or with pos_active_host 0.  0: one body-only step per position (B rows each, the whole body
 * weight set streamed n0 times).  1, with n0 >= 1 and some position to draw: tokens 0 .. block_size_cond - 1 + n0 - 2 of every row
 * -- the conditioning tokens, then the embeddings of positions 0 .. n0 - 2 -- go through the body stack in ONE pass (rows chunked by
 * "fwd.chunk_rows", in the one-pass forward's workspace; a guided call prefills both twins, each under its own conditioning), the
 * position counter is set to n0 and the usual loop goes on from there.  For a text-conditioned model the pass replaces the
 * text-only prefill.  Later positions see the same arithmetic through other GEMM tiles: logits differ by rounding, so a draw that was
 * close may come out differently -- filters and Philox counters are the same.  Captured graphs are shared by the two settings; model
 * log-probabilities stay NaN and draw +0.0 at the prefix positions.  Kept runs that are not leading stay stepped (see below).
 * "masked.run_prefill" (0 | 1, default 0; additive, ABI v7): how the same entry points bring kept runs that are NOT leading into the
 * cache.  A position is inactive when no head runs there: it lies before start_h / start_w, or pos_active_host is 0.  0: one body-only
 * step per inactive position.  1: every maximal run [p0, p1) of inactive positions behind position 0 and behind what "prefix.one_pass"
 * covered, of two positions at least and with a drawn position after it (p1 < the end of the last active position), goes through the
 * body stack in ONE pass: R = p1 - p0 tokens per row -- the embeddings of the codes at p0-1 .. p1-2 with their positional entries --
 * whose keys / values are appended at cache rows block_size_cond - 1 + p0 .. + p1 - 1 behind the rows the earlier positions wrote
 * (csrc/rqt_attn_extend.hip), rows chunked by "fwd.chunk_rows" in the one-pass forward's workspace; the position counter is set to p1
 * and the usual loop goes on there.  Guided and composed calls run all their (2 + n_extra) * batch rows through the pass.  Position 0 is
 * always stepped (its input is the conditioning token), so with "prefix.one_pass" off a leading run is position 0 stepped and positions
 * 1 .. n0-1 in one pass.  Stepped as before, silently: runs of one position, RQAMD_KV=int8k / int8kv handles, body head sizes other
 * than 64, shared-prompt calls (rqamd_rqt_sample_shared).  Numerics and graphs as for "prefix.one_pass": same arithmetic through other
 * GEMM tiles, the same captured graphs in both settings. */
int rqamd_rqt_set_option(rqamd_rqt* h, const char* name, int value);
int rqamd_rqt_set_param(rqamd_rqt* h, const char* name, const float* dev_ptr, const int64_t* shape,
                        int ndim, void* stream);
/* rqamd_rqt_sample <- RQTransformer.sample (transformers.py:294-369) with cached=True:
 * partial (batch,H,W,D) int64 (not modified); cond (batch, block_size_cond) int64 or NULL (zeros);
 * codebooks[d] (n_embed, input_embed_dim) fp32 without padding row (model_aux.get_code_emb_with_depth);
 * top_k[D] / top_p[D] per-depth lists already normalised as transformers.py:314-330 does;
 * codes_out (batch,H,W,D) int64.  use_graph != 0 replays one captured hipGraph per (h,w). */
int rqamd_rqt_sample(rqamd_rqt* h, const int64_t* partial, const int64_t* cond, int batch,
                     const float* const* codebooks, int start_h, int start_w, float temperature,
                     const int* top_k, const float* top_p, uint64_t seed, uint64_t offset,
                     int use_graph, int64_t* codes_out, void* stream);
/* Masked form of rqamd_rqt_sample (inpainting, outpainting, depth refinement, a region per image); additive, ABI v7.
 * keep (batch,H,W,D) bytes on the DEVICE, nonzero = the code is kept: it stays as `partial` gives it and everything drawn later is
 * conditioned on it.  Every other code is drawn as rqamd_rqt_sample draws it (same logits, filter and Philox counter
 * offset + pos * D + d of its row); its value in `partial` is never read.  With the seed and offset of an unmasked call and kept
 * codes equal to what that call drew, the result is that call's, bit for bit.  `keep` is copied into the handle when the call
 * starts: the caller may free it once the stream has reached that point, and captured graphs never hold it.
 * pos_active_host: H * W bytes on the HOST or NULL (every position active).  0 at position p is the caller's promise that
 * every code of p is kept in every row: p then runs the body stack only, as the positions before start_h / start_w do, and
 * nothing runs after the last active position.  There is no start_h / start_w: a kept prefix is part of `keep`.
 * Masked calls replay captured graphs of their own: alternating with rqamd_rqt_sample recaptures nothing. */
int rqamd_rqt_sample_masked(rqamd_rqt* h, const int64_t* partial, const uint8_t* keep, const uint8_t* pos_active_host,
                            const int64_t* cond, int batch, const float* const* codebooks, float temperature,
                            const int* top_k, const float* top_p, uint64_t seed, uint64_t offset,
                            int use_graph, int64_t* codes_out, void* stream);
/* Classifier-free guidance inside the engine (not in the reference); additive, ABI v7.  The `batch` images run as 2 * batch rows:
 * row b under cond[b], row batch + b under uncond[b] (NULL = zeros, as for cond), both started from the same `partial` (and `keep`).
 * At every step the classifier gives the logits of all 2 * batch rows; row b is then drawn from
 *     g = guide(c, u, s) = (c == -inf) ? -inf : fmaf(s - 1, c - u, c),   c = logits[b], u = logits[batch + b], s = guidance_scale
 * (fp32, raw logits, before the temperature; u + s (c - u), written so that s = 1 returns c bit for bit) with the temperature,
 * top-k, top-p and Philox counter offset + pos * D + d of row b of an unguided call, and the code is written to both rows: the
 * unconditional twin sees exactly what its conditional twin drew.  codes_out (batch,H,W,D): rows 0 .. batch - 1.
 * Which GEMM and attention kernels a row takes follows the 2 * batch rows of the step; s = 1 runs the pairs like any other scale
 * and returns what rqamd_rqt_sample over the 2 * batch rows (partial twice, cond then uncond) returns in its first half.
 * keep / pos_active_host: as in rqamd_rqt_sample_masked (batch rows of flags; row b's flags hold for both twins), or NULL: nothing
 * kept (pos_active_host is then ignored).  start_h / start_w as in rqamd_rqt_sample; a masked call passes 0, 0.
 * Any finite guidance_scale is accepted (0 draws from the unconditional rows, negative values push away from cond); NaN or
 * infinity: RQAMD_ERR_INVALID.  Guided calls replay captured graphs of their own (masked and unmasked), keyed on 2 * batch and on
 * guidance_scale next to the fields of the unguided key: alternating with unguided calls recaptures nothing, a new scale recaptures
 * the guided graphs only. */
int rqamd_rqt_sample_guided(rqamd_rqt* h, const int64_t* partial, const uint8_t* keep, const uint8_t* pos_active_host,
                            const int64_t* cond, const int64_t* uncond, int batch, const float* const* codebooks,
                            int start_h, int start_w, float temperature, float guidance_scale, const int* top_k,
                            const float* top_p, uint64_t seed, uint64_t offset, int use_graph, int64_t* codes_out, void* stream);
/* out[r][v] = guide(cond_logits[r][v], uncond_logits[r][v], scale) of rqamd_rqt_sample_guided, through the same device function:
 * (rows, vocab) fp32, contiguous, device memory; vocab >= 1 (16-byte accesses when vocab % 4 == 0 and the three bases are aligned).
 * For host-driven loops (rqamd_rqt_step_logits over 2 * batch rows) and for tests; the engine never materialises g. */
int rqamd_guide_logits(const float* cond_logits, const float* uncond_logits, int rows, int vocab, float scale, float* out, void* stream);
/* Composed guidance: negative prompts and extra conditions inside the engine (not in the reference); additive, ABI v7.  Arms the NEXT
 * rqamd_rqt_sample_guided call, or guided rqamd_rqt_sample_rows call, on the handle; that call consumes the arming whether it
 * succeeds or fails.  n_extra = 0 disarms.  extra_cond: n_extra DEVICE pointers to (batch, block_size_cond) int64 each, a NULL entry
 * (or a NULL array) = zeros as for cond; the pointer array is copied when the call arms, the conditionings are read by the armed call.
 * extra_weight: HOST array of n_extra * batch finite values, condition-major (weight of condition k for image b at [k * batch + b]),
 * read by the armed call.  The `batch` images then run as (2 + n_extra) * batch rows: row b under cond[b], row batch + b under uncond[b],
 * row (2 + k) * batch + b under extra_cond[k][b], all started from the same `partial` and `keep`.  With c, u and x_k the raw logits of
 * those rows and w_k = extra_weight[k * batch + b], every code of image b is drawn from
 *     G = u + s (c - u) + sum_k w_k (x_k - u)
 * -- a negative prompt is an extra condition with w < 0, a second prompt one with w > 0 -- computed in fp32 as
 *     e = 0;  for k = 0 .. n_extra - 1:  e = fmaf(w_k, x_k - u, e)
 *     (c == -inf || e == 0) ?  c' = c, u' = u  :  c' = c + e, u' = u + e;        g = guide(c', u', s)
 * with guide() of rqamd_rqt_sample_guided.  Columns LogitMask holds at -inf in every row stay -inf (never inf - inf); e == 0 -- every
 * weight zero, or every extra row equal to the unconditional one -- leaves the pair untouched bit for bit, so such a call draws what
 * the guided call over the same (2 + n_extra) * batch rows would.  The fold is one launch per head step (csrc/rqt_compose.hip) into a
 * scratch of the handle; the sampler kernels, filters, temperature and Philox counters are those of the guided call, and the code is
 * written to all 2 + n_extra rows of the image.  It composes with rqamd_rqt_sample_logp (draw: under the composed distribution;
 * model / model_uncond: the raw logits of rows b and batch + b, as without extra conditions), _trunc and _schedule (a guidance
 * schedule applies to s alone; the weights have no schedule), keep, start_h / start_w and "prefix.one_pass".
 * Composed calls replay graph sets of their own, keyed on the rows and n_extra next to the fields of the family the call would
 * otherwise belong to; the weights live in a device table and are in no key: alternating composed, guided and plain calls recaptures
 * nothing, new weights recapture nothing, another n_extra recaptures the composed sets only.
 * Refused before anything is enqueued, RQAMD_ERR_INVALID: n_extra outside 0 .. RQAMD_RQT_MAX_EXTRA_CONDS (by this call), a NaN or
 * infinite weight, an arming in front of an unguided call; RQAMD_ERR_UNSUPPORTED: an arming together with rqamd_rqt_sample_shared. */
#define RQAMD_RQT_MAX_EXTRA_CONDS 4
int rqamd_rqt_sample_compose(rqamd_rqt* h, int n_extra, const int64_t* const* extra_cond, const float* extra_weight);
/* out[r][v] = guide(c', u', scale) of rqamd_rqt_sample_compose, through the same device function: cond_logits, uncond_logits, out
 * (rows, vocab) fp32, extra_logits (n_extra, rows, vocab) fp32, extra_weight (n_extra, rows) fp32, all contiguous DEVICE memory;
 * 1 <= n_extra <= RQAMD_RQT_MAX_EXTRA_CONDS, vocab >= 1 (16-byte accesses when vocab % 4 == 0 and the bases are aligned).  For
 * host-driven loops over (2 + n_extra) * batch rows and for tests; the engine folds into its own scratch and never calls it. */
int rqamd_compose_logits(const float* cond_logits, const float* uncond_logits, const float* extra_logits, int n_extra,
                         const float* extra_weight, int rows, int vocab, float scale, float* out, void* stream);
/* Anchored sampling: draw codes near an encoded image inside the engine (not in the reference); additive, ABI v7.  Arms the NEXT
 * rqamd_rqt_sample, _masked, _guided or _rows call on the handle; that call consumes the arming whether it succeeds or fails.
 * z = NULL disarms.  z: DEVICE, (batch, H, W, dim) fp32, the output of RQVAE.encode in code shape, copied into the handle by the armed
 * call.  codebooks / code_norms: D DEVICE pointers each (the two pointer arrays are copied when the call arms), every codebook exactly
 * `vocab_size` codes of width dim and 16-byte aligned like z, the norms from rqamd_rq_code_norms.  weight: HOST array of H * W * D values >= 0 (per_image = 0: one
 * table for all images) or batch * H * W * D values (per_image = 1, image-major, depth last), read and checked by the armed call.
 * At every head step the logits of image b get the quantiser's soft-code term of the residual the image has at that depth given the
 * codes drawn (or kept) so far:
 *     x'[v] = x[v] - w(b, p, d) * dist(r_d(b, p), codebook_d[v]),    r_0 = z[b, p, :],   r_{d+1} = r_d - codebook_d[code(b, p, d)]
 * dist the expanded-form squared distance in fp32 (the values of rqamd_rq_distances over the same rows, bit for bit), the residual
 * subtracted one depth after the other in fp32 as rqamd_rq_quantize does.  w = 0 is the prior, w -> inf the codes of rqamd_rq_quantize, and
 * in between the distribution is p_model * softmax(-dist / temp) with w = 1 / temp: get_soft_codes as a likelihood.  In fp32,
 *     x' = (x == -inf || w == 0 || dist is not finite) ? x : fmaf(-w, dist, x)
 * -- LogitMask columns stay -inf; w == 0 leaves the logit bit for bit (-0.0 included), so an all-zero table draws what the unarmed call
 * draws; a distance that is NaN or infinite (a non-finite z row; never with finite z) leaves the logit alone, so that image degrades to
 * unanchored.  Guided calls: both twins of a pair get the same term before guide(), so the guided mix is shifted by -w * dist up to
 * rounding.  Three launches per head step (csrc/rqt_anchor.hip: residual, the quantiser's distance kernel, fold) into memory of the
 * handle; the sampler kernels, filters, temperature and Philox counters are those of the unarmed call.  It composes with keep (the
 * residual follows the given code), start_h / start_w, "prefix.one_pass" and "masked.run_prefill" (no head step, no anchor), per-image
 * parameters and seeds, rqamd_rqt_sample_logp (draw: under the anchored distribution after all stages; model / model_uncond: the raw
 * logits, as without an anchor), _trunc and _schedule.
 * Anchored calls replay graph sets of their own, keyed on the codebook and norms pointers and dim next to the fields of the family the
 * call would otherwise belong to; z and the weights live in memory of the handle and are in no key: alternating anchored and plain
 * calls recaptures nothing, a new z or new weights recapture nothing.
 * Refused before anything is enqueued, RQAMD_ERR_INVALID: a weight that is negative or not finite, null weights, a null codebook or
 * norms pointer; RQAMD_ERR_UNSUPPORTED: dim other than 64 / 128 / 192 / 256, depths with different vocabularies (vocab_sizes[d] <
 * vocab_size), an arming together with rqamd_rqt_sample_shared or rqamd_rqt_sample_compose. */
int rqamd_rqt_sample_anchor(rqamd_rqt* h, const float* z, const float* const* codebooks, const float* const* code_norms, int dim,
                            const float* weight, int per_image);
/* The three stages of ONE anchored step over given rows, through the kernels and the device function of rqamd_rqt_sample_anchor: for
 * host-driven loops and for tests.  logits, out (rows, vocab) fp32; logits_u / out_u the unconditional twins, both or neither; z_rows
 * (rows, dim) fp32 and 16-byte aligned; codes (rows, d) int64, the codes of depths 0 .. d-1 (NULL with d = 0; a code outside
 * 0 .. vocab-1 traps); codebooks / code_norms: d + 1 DEVICE pointers each, `vocab` codes of width dim (64 / 128 / 192 / 256), the
 * codebooks 16-byte aligned (RQAMD_ERR_INVALID otherwise, as for z_rows and resid_out); weight:
 * DEVICE, rows values (not checked).  resid_out (rows, dim) and dist_out (rows, vocab), each or NULL: the residual and the distances of
 * the step.  workspace: 16-byte aligned DEVICE memory, 256-byte rounded rows * 512 bytes, plus rows * dim * 4 (256-byte rounded) without
 * resid_out, plus rows * vocab * 4 without dist_out.  All contiguous device memory; 16-byte accesses in the fold when vocab % 4 == 0
 * and the bases are aligned. */
int rqamd_anchor_logits(const float* logits, const float* logits_u, const float* z_rows, const int64_t* codes,
                        const float* const* codebooks, const float* const* code_norms, int d, int dim, int vocab, const float* weight,
                        int rows, float* out, float* out_u, float* resid_out, float* dist_out, void* workspace, int64_t workspace_bytes,
                        void* stream);
/* Sampling parameters per image (not in the reference); additive, ABI v7.  One entry point for plain, masked and guided sampling:
 * keep NULL: unmasked (pos_active_host is ignored), else as in rqamd_rqt_sample_masked; uncond NULL and guidance_scale NULL: unguided,
 * else as in rqamd_rqt_sample_guided (uncond NULL = zeros; uncond without guidance_scale is RQAMD_ERR_INVALID).
 * HOST arrays, read before the call returns: temperature (batch), top_k and top_p (batch * D, image-major: [b * D + d]),
 * guidance_scale (batch) or NULL, seeds (batch) or NULL.  Every temperature must be > 0 and finite and every scale finite, else
 * RQAMD_ERR_INVALID; top_k <= 0 or >= vocab and top_p < 0 mean "off" (top_p = 1.0 keeps every token), as elsewhere.
 * Image b is drawn exactly as the scalar entry point draws row b of the same batch with b's values: the same logits, the sampler
 * kernel those values select, the same Philox counters -- bit for bit, whatever the other rows ask for.
 * seeds NULL: key `seed`, counter offset + pos * D + d and Philox row b, as in the scalar calls.  seeds given: image b draws with key
 * seeds[b], Philox row 0 and counter pos * D + d, the stream of row 0 of a scalar call seeded with seeds[b] at offset 0, wherever the
 * image stands in the batch (seed / offset are then unused).
 * The values live in device buffers of the handle that the sampler kernels read, so the captured graphs of per-row calls (four sets
 * of their own: plain, masked, guided, guided + masked; four more for calls with seeds, whose sampler launches take their key from
 * another buffer) are keyed on rows, codebooks, stream and the guided flag only: a call with other values replays them, and scalar,
 * per-row and seeded per-row calls never invalidate or replay each other's graphs. */
int rqamd_rqt_sample_rows(rqamd_rqt* h, const int64_t* partial, const uint8_t* keep, const uint8_t* pos_active_host,
                          const int64_t* cond, const int64_t* uncond, int batch, const float* const* codebooks,
                          int start_h, int start_w, const float* temperature, const int* top_k, const float* top_p,
                          const float* guidance_scale, const uint64_t* seeds, uint64_t seed, uint64_t offset,
                          int use_graph, int64_t* codes_out, void* stream);
/* Log-probabilities of the draws (not in the reference); additive, ABI v7.  Arms the NEXT rqamd_rqt_sample, _masked, _guided or
 * _rows call on the handle; that call consumes the arming whether it succeeds or fails.  Each output is a device pointer to
 * (batch, H, W, D) fp32 or NULL; all NULL disarms.  The armed call returns, bit for bit, the codes of the unarmed call with the same
 * arguments, seed and offset, and after it
 *   draw[b,h,w,d]   = log of the probability, in the distribution the draw was made from (logits after guidance, temperature, top-k,
 *                     top-p and renormalisation), of the code that was drawn; +0.0 for every code that was not drawn (kept codes,
 *                     codes before start_h / start_w);
 *   model[b,h,w,d]  = log_softmax of row b's raw logits (before guidance and temperature, per-depth vocabulary mask applied) at the
 *                     code, drawn or kept; NaN where the head stack did not run (positions before the start, positions that
 *                     pos_active_host promises away);
 *   model_uncond    = the same for the unconditional twin rows batch + b; with an unguided call it is RQAMD_ERR_INVALID.
 * The values are written into the handle's workspace and copied out next to codes_out, so captured graphs never hold a caller's
 * pointer.  Armed calls replay graph sets of their own: alternating armed and unarmed calls recaptures nothing. */
int rqamd_rqt_sample_logp(rqamd_rqt* h, float* draw_logp_out, float* model_logp_out, float* model_logp_uncond_out);
/* Min-p and locally typical sampling in the engine (the stages of rqamd_sample_logits_trunc); additive, ABI v7.  Arms the NEXT
 * rqamd_rqt_sample, _masked, _guided or _rows call on the handle; that call consumes the arming whether it succeeds or fails, and
 * reads the arrays: HOST arrays of D values (one per depth), or -- per_image = 1, valid in front of rqamd_rqt_sample_rows only, else
 * that call returns RQAMD_ERR_INVALID -- of batch * D values, image-major.  Either pointer NULL: that filter is off; both NULL
 * disarms.  A non-finite value or a min_p above 1 makes the armed call RQAMD_ERR_INVALID.  It combines freely with
 * rqamd_rqt_sample_logp: draw is then the log of the probability after all stages.  A scalar call whose every value is off is the
 * unarmed call; a depth whose two values are off launches what it launches unarmed.  Calls with a filter in effect replay graph
 * sets of their own (scalar values are part of their key, per-image values live in tables of the handle and a new set of values
 * replays the same graphs): alternating armed and unarmed calls recaptures nothing. */
int rqamd_rqt_sample_trunc(rqamd_rqt* h, const float* min_p, const float* typical_p, int per_image);
/* Sampling schedules over positions and depths (not in the reference); additive, ABI v7.  Arms the NEXT rqamd_rqt_sample, _masked,
 * _guided or _rows call on the handle; that call consumes the arming whether it succeeds or fails, and reads the arrays: HOST arrays
 * of H * W * D values in raster order, depth last (per_image = 0: one schedule for every image), or of batch * H * W * D values,
 * image-major (per_image = 1; valid in front of any of the four).  A NULL pointer: that parameter comes from the armed call's own
 * arguments (a number, per-depth values, per-image values, or an arming of rqamd_rqt_sample_trunc), broadcast over the positions; all
 * NULL disarms.  Code (b, p, d) is then drawn, bit for bit, as rqamd_sample_logits_rows -- rqamd_sample_logits_trunc where a min-p /
 * typical value is on there -- draws row b from the same logits (the guided mix with the scale at (b, p, d) included) with the values
 * at (b, p, d); Philox key, row field and counter offset + p * D + d are those of the unarmed call (per-image seeds: of
 * rqamd_rqt_sample_rows).  So a schedule that is constant over the positions returns the per-image call's codes, and the scalar
 * call's.  top_k <= 0 or >= vocab, top_p < 0 or >= 1, min_p <= 0 and typical_p < 0 or >= 1 are off, as in the per-row arrays.
 * The armed call checks the values on the host before anything is enqueued: a temperature that is not finite and > 0, a non-finite
 * guidance scale, min_p or typical_p, a min_p above 1, or a guidance schedule in front of an unguided call make it
 * RQAMD_ERR_INVALID, and nothing is written.  Kept codes, start_h / start_w, pos_active_host, "prefix.one_pass" and the two other
 * armings behave as without a schedule (draw: the log-probability after all stages, with the values of the position).
 * The values live in device tables of the handle -- H * W * D entries each for a shared schedule, batch * H * W * D (allocated at
 * the first such call and kept) when the schedule or any argument is per image -- which the sampler kernels index with the position
 * they read from the device.  Scheduled calls always take the per-row launch sequence and replay graph sets of their own, whose keys
 * hold no value: another schedule replays the same graphs, and scheduled, per-image and scalar calls never recapture each other's. */
int rqamd_rqt_sample_schedule(rqamd_rqt* h, const float* temperature, const int* top_k, const float* top_p,
                              const float* guidance_scale, const float* min_p, const float* typical_p, int per_image);
/* Shared-prompt sampling (N images per prompt on one cached text prefix; not in the reference); additive, ABI v7.  Arms the NEXT
 * rqamd_rqt_sample, _masked, _guided or _rows call on the handle; that call consumes the arming whether it succeeds or fails.
 * fan = 0 disarms.  In the armed call `batch` = G * fan rows, `cond` / `uncond` hold G = batch / fan rows; row r belongs to group
 * r / fan (guided: the unconditional twin batch + r to group G + r / fan).  Row r is drawn as the unarmed call with every cond row
 * repeated fan times draws it: the same decode-step, sampler and Philox launches over `batch` rows.  Only the prefix keys and values
 * differ in origin: they come out of a prefill over G * (block_size_cond - 1) rows instead of batch * (block_size_cond - 1), so the
 * codes are bit-identical wherever the two prefills fall into one GEMM regime and differ only where a draw was close
 * elsewhere.  The body stack's KV workspace is then laid out as one group cache of block_size_cond - 1 slots per (group, head) --
 * ordinary cached memory -- plus H * W own slots per (row, head); the decode attention of the body stack reads the group's slots
 * from the one copy (csrc/rqt_attn_shared.hip).  A handle's KV workspace has one layout at a time: a call in the other form re-lays it
 * and drops the captured graphs.  Shared calls replay graph sets of their own; a second shared call with other prompts captures
 * nothing.  The text prefix always goes through the shared prefill; given code positions are stepped, whatever "prefix.one_pass"
 * says.  It composes with rqamd_rqt_sample_logp, _trunc and _schedule.
 * Refused before anything is enqueued: fan < 0 or batch % fan != 0: RQAMD_ERR_INVALID; block_size_cond < 2 (nothing to share),
 * RQAMD_KV=int8k / int8kv, a body context over 256 or a body head size other than 64: RQAMD_ERR_UNSUPPORTED. */
int rqamd_rqt_sample_shared(rqamd_rqt* h, int fan);
/* *bytes = the device bytes currently reserved for the KV caches of the handle (0 before the first batch).  A reservation, not the need
 * of the last call: within one layout the caches only grow, so after shared calls the figure covers the largest batch and the largest
 * group count seen since the layout was last laid out (a call in the other form starts again from its own sizes). */
int rqamd_rqt_kv_bytes(rqamd_rqt* h, int64_t* bytes);
/* *captures = the number of position graphs this handle has captured so far (every form of sampling); a call that replays only
 * leaves it unchanged. */
int rqamd_rqt_graph_captures(rqamd_rqt* h, int64_t* captures);
/* rqamd_rqt_logits <- the same cached_forward stepping (transformers.py:190-287) driven
 * teacher-forced over given codes, returning every step's logits: logits_out (batch,H,W,D,vocab) fp32.
 * This is the parity hook against RQTransformer.forward (transformers.py:113-188). */
int rqamd_rqt_logits(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch,
                     const float* const* codebooks, float* logits_out, void* stream);
/* rqamd_rqt_forward <- RQTransformer.forward (transformers.py:113-188) including the text-conditioned return value
 * (seq_logits, cond_logits) (:150-153,:185-186): as rqamd_rqt_logits, plus cond_logits_out (batch, block_size_cond-1,
 * vocab_size_cond) fp32 = cond_classifier over the body outputs of the conditioning prefix (NULL to skip; must be NULL
 * when block_size_cond <= 1). */
int rqamd_rqt_forward(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch,
                      const float* const* codebooks, float* logits_out, float* cond_logits_out, void* stream);
/* RQTransformer.forward (transformers.py:113-188) in ONE pass over all positions; outputs as rqamd_rqt_forward.  Every code is
 * given, so the body stack runs once over (image, token) rows and the head stack once over (image, position, depth) rows with
 * cache-free causal attention; no KV cache is used.  The work is chunked by rows (rqamd_rqt_set_option "fwd.chunk_rows", default
 * 4096) in a workspace of its own: captured sampling graphs of the handle stay valid.  Same arithmetic as the stepped entry points;
 * results differ from theirs by the GEMM tile choice only. */
int rqamd_rqt_forward_onepass(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch,
                              const float* const* codebooks, float* logits_out, float* cond_logits_out, void* stream);
/* log p(code) of every code under the same pass: logp_out (batch,H,W,D) fp32 = log_softmax(logits)[code], reduced from
 * sub-chunks of logits rows in the workspace -- (batch,H,W,D,vocab) is never materialised.  cond_logp_out (batch,
 * block_size_cond-1) fp32 = log p(cond[t+1] | cond[:t+1]) under cond_classifier, or NULL (must be NULL when block_size_cond <= 1;
 * needs cond).  A code outside 0..vocab-1 gives NaN. */
int rqamd_rqt_log_probs(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch,
                        const float* const* codebooks, float* logp_out, float* cond_logp_out, void* stream);
/* Soft-target cross entropy of every code under the same pass (additive, ABI v7): loss_out (batch,H,W,D) fp32 =
 * soft_target_cross_entropy(logits, soft targets, reduction='none') (rqvae/optimizer/loss.py:68-84), what compute_loss /
 * compute_codebook_loss (transformers.py:371-410) average with use_soft_target -- reduced from the sub-chunks of logits rows
 * rqamd_rqt_log_probs uses (rqamd_rqt_set_option "fwd.logits_bytes", default 48 << 20, at least one depth group), so
 * (batch,H,W,D,vocab) logits never exist.  Exactly one of
 *   soft_targets (batch,H,W,D,vocab) fp32: the soft codes of RQBottleneck.get_soft_codes (quantizations.py:371-400), or any weights;
 *   z (batch,H,W,input_embed_dim) fp32: the features the codes were quantised from, with code_norms[d] (vocab) from
 *     rqamd_rq_code_norms and temp > 0 -- the targets softmax(-distance(residual_d, codebook_d) / temp) are formed per sub-chunk
 *     from the residual of the GIVEN codes (argmin or drawn) and never stored; codebooks[d] must hold exactly `vocab` codes.
 * All depths must share one vocabulary (RQAMD_ERR_UNSUPPORTED otherwise); with z, input_embed_dim is 64, 128, 192 or 256.
 * cond_logp_out: as rqamd_rqt_log_probs. */
int rqamd_rqt_soft_loss(rqamd_rqt* h, const int64_t* codes, const int64_t* cond, int batch, const float* const* codebooks,
                        const float* soft_targets, const float* z, const float* const* code_norms, float temp, float* loss_out,
                        float* cond_logp_out, void* stream);
/* Stepping form of rqamd_rqt_sample for callers that draw the samples themselves -- e.g. torch.multinomial on the filtered
 * probabilities, which consumes the device generator exactly as the reference's sample_from_logits does
 * (rqvae/utils/utils.py:112; RQTransformer.sample transformers.py:346-364 is this loop):
 *   step_begin     copies partial / cond into the handle, runs the conditioning prefix; codebooks as for rqamd_rqt_sample
 *                  (the pointer ARRAY is copied, the codebooks must stay alive until step_end)
 *   step_logits    logits (batch, vocab_size) fp32 of step (pos, d) given the codes written so far; steps must come in order
 *                  (pos ascending, d = 0..D-1); d < 0 runs only the body stack of that position (positions before start_loc,
 *                  whose codes are given: KV cache only).  *logits_dev points into the handle's workspace and is valid until
 *                  the next call on the handle.  Columns >= vocab_sizes[d] are masked to -inf (LogitMask).
 *   step_prefill   (additive, ABI v7) valid only directly after step_begin, else RQAMD_ERR_STATE: fills the KV cache for positions
 *                  0 .. n_pos-1 in one pass over the codes of `partial` (see "prefix.one_pass"; the option is not consulted).  Stands
 *                  for step_logits(p, -1), p < n_pos: the next step_logits must be (n_pos, 0) or (n_pos, -1).  n_pos outside
 *                  1 .. H*W-1: RQAMD_ERR_INVALID
 *   step_run       (additive, ABI v7) stands for step_logits(p, -1), p0 <= p < p1, in one pass over the codes of positions
 *                  p0-1 .. p1-2 (see "masked.run_prefill"; the option is not consulted; a handle the pass does not serve -- 8-bit
 *                  cache, body head size other than 64 -- takes the steps themselves).  Valid only when the sequence stands at position
 *                  p0 with no head step of p0 taken, else RQAMD_ERR_STATE; p0 < 1, p1 <= p0 or p1 > H*W-1: RQAMD_ERR_INVALID.  The
 *                  next step_logits must be (p1, 0) or (p1, -1)
 *   step_set_code  writes codes[batch] as code (pos, d) of every image
 *   step_end       copies the codes (batch,H,W,D) out (codes_out may be NULL) and ends the sequence.
 * Any other call on the handle ends a sequence in progress. */
int rqamd_rqt_step_begin(rqamd_rqt* h, const int64_t* partial, const int64_t* cond, int batch,
                         const float* const* codebooks, void* stream);
int rqamd_rqt_step_prefill(rqamd_rqt* h, int n_pos, void* stream);
int rqamd_rqt_step_run(rqamd_rqt* h, int p0, int p1, void* stream);
int rqamd_rqt_step_logits(rqamd_rqt* h, int pos, int d, const float** logits_dev, void* stream);
int rqamd_rqt_step_set_code(rqamd_rqt* h, int pos, int d, const int64_t* codes, void* stream);
int rqamd_rqt_step_end(rqamd_rqt* h, int64_t* codes_out, void* stream);
/* timing hook for bench.py: average device time (ms) of the engine's weight-streaming GEMM launches
 * during the last rqamd_rqt_sample call is not observable from outside the stream, so the engine can
 * bracket every GEMM launch of one call with HIP events (profile != 0 disables graphs for that call). */
int rqamd_rqt_set_profile(rqamd_rqt* h, int profile);   /* 0 off; 1 events around every GEMM / attention launch (eager); 2 skip the
                                                          * GEMM launches (graphs on): pass time minus this = the GEMMs' time in situ */
int rqamd_rqt_get_profile(rqamd_rqt* h, double* gemm_ms_total, int64_t* gemm_launches,
                          double* gemm_bytes_total, double* gemm_flops_total);
/* the cached-attention launches (MultiSelfAttention.forward with the KV cache, attentions.py:60-104) of the same profiled call:
 * total device time and launch count (the KV bytes they read are a function of the shapes: bench.py computes them). */
int rqamd_rqt_get_profile_attn(rqamd_rqt* h, double* attn_ms_total, int64_t* attn_launches);

/* ---- diagnostics ------------------------------------------------------------------------------
 * One raw launch of the engines' bf16 MFMA GEMM: out[M,N] = A[M,K] . W[N,K]^T (+bias), both operands bf16
 * K-contiguous (W = nn.Linear.weight layout).  epi: 0 bf16 out, 1 bf16 + GELU, 3 fp32 out, 4 fp32 split-K
 * partial slabs out[splitk][M][N] (no bias); + 16: skip the epilogue (ablation); + 64 / + 96: stage the operands by
 * LDS-DMA through 2 / 3 LDS stages (tiles 128x64, 128x128, 256x128); 4 + 2048 (splitk 1): update out[M][N] in place,
 * out = (out + A.W^T) + bias -- the residual-stream epilogue of the decode step.  bm/bn <= 0: the engine's own tile choice.
 * Used by the kernel-level parity test and scripts/gemm_bench.py; not part of the reference-facing surface. */
int rqamd_dbg_gemm_bf16(const void* A, const void* W, int M, int N, int K, const float* bias, int epi,
                        void* out, int bm, int bn, int splitk, void* stream);
/* One raw implicit-GEMM convolution launch (the conv form of the same kernel): x NHWC bf16
 * [B][H>>ups][W>>ups][Cin] (H, W = virtual input size after the folded nearest-2x upsample), w bf16
 * [Cout][k][k][Cin], out NHWC bf16 (+bias, +resid if not NULL); stride 2 = Downsample (layers.py:50-54).
 * flags bit 0: skip the epilogue (ablation); bits 8..12: virtual split-K count (the K loop as that many chunks, each summed
 * from zero and added in chunk order -- what the engine runs on its <= 32^2 convs of many images; 0 or 1 = none; the count
 * must leave an even number of K-tiles per chunk). */
int rqamd_dbg_conv_bf16(const void* x, const void* w, const float* bias, const void* resid, int B, int H, int W,
                        int Cin, int Cout, int ksize, int stride, int ups, void* out, int bm, int bn, int flags,
                        void* stream);

/* One launch of the halo-reuse 3x3 / stride-1 conv used for the high-resolution decoder/encoder layers
 * (csrc/conv_halo.hip): x NHWC bf16 [B][H][W][Cin], w bf16 [Cout][3][3][Cin], out NHWC bf16; gn = NULL or fp32
 * [B][Cin][2] (scale, shift): the input is then read as silu(x*scale + shift), i.e. GroupNorm+SiLU fused into the
 * staging (ResnetBlock norm -> swish -> conv, layers.py:100-120).  stats = NULL or fp32 [B][(H/8)*(W/32)][32][2]:
 * per-tile (sum, sum of squares) of the 32 GroupNorm groups of `out` (Cout 128/256/512), taken in the epilogue for
 * the next layer's Normalize.  ups != 0: x is [B][H/2][W/2][Cin], read through the nearest 2x upsample of
 * Upsample.forward (layers.py:31-35; gn and resid must be NULL).  Needs H % 8 == 0, W % 32 == 0, H >= 64,
 * Cin % 64 == 0, Cout % 128 == 0. */
int rqamd_dbg_conv_halo_bf16(const void* x, const void* w, const float* bias, const float* gn, const void* resid,
                             int B, int H, int W, int Cin, int Cout, int ups, void* out, float* stats, void* stream);

/* One launch of the MFMA Decoder.conv_out kernel (modules.py:165-169): x NHWC bf16 [B][H][W][Cin], w fp32
 * [Cout][3][3][Cin] (Cout <= 4), y NCHW fp32 [B][Cout][H][W]; gn as above (norm_out + swish fused into the
 * staging).  Needs H % 4 == 0, W % 32 == 0, Cin in {64, 128, 256}. */
/* diagnostics: w (Cout,3,3,Cin) bf16 -> wsub (4,Cout,2,2,Cin) bf16, the pre-summed weights of the sub-pixel form of Upsample.conv
 * (layers.py:20-35: nearest 2x + 3x3 conv = four 2x2 convs over the source image); rqamd_dbg_conv_halo_bf16 takes them with ups bit 6 set */
int rqamd_dbg_ups_subpixel_weights(const void* w, int Cout, int Cin, void* wsub, void* stream);
int rqamd_dbg_conv_out_bf16(const void* x, const float* w, const float* bias, const float* gn, int B, int H, int W,
                            int Cin, int Cout, float* y, void* stream);

/* One launch of the MFMA Encoder.conv_in kernel (modules.py:23-27): x NCHW fp32 [B][3][H][W], w fp32 [3][3][3][128]
 * = (ky, kx, ci, cout), y NHWC bf16 [B][H][W][128].  Needs H % 8 == 0, W % 32 == 0. */
int rqamd_dbg_conv_in_bf16(const float* x, const float* w, const float* bias, int B, int H, int W, void* y, void* stream);

/* One launch of the single-head spatial attention of AttnBlock (layers.py:158-182): qkv bf16 [B*T][3C] (q | k | v per token) ->
 * out bf16 [B*T][C] = softmax(q k^T C^-0.5) v per image.  form: 0 the engine's own choice, 1 the wavefront-per-query kernel (T <= 1024),
 * 2 the 64-token MFMA kernel (T == 64), 3 the tiled MFMA kernel (T % 64 == 0, 128 <= T <= 4096); forms 2 and 3 need C % 64 == 0,
 * C <= 512.  A (form, shape) pair outside these limits returns RQAMD_ERR_UNSUPPORTED. */
int rqamd_dbg_vae_attn(const void* qkv, int B, int T, int C, int form, void* out, void* stream);

/* The RQ-Transformer's attention launchers alone (csrc/rqt_kernels.hip), for the stand-alone fp64 checks of tests/rqt_attn_cases.py: each
 * entry fills the launcher's argument struct and calls it unchanged, so the kernel is the one the engine would pick for these sizes
 * (rqamd_dbg_set_row_scale and the RQAMD_ATTN_LONG / RQAMD_ATTN_LONG_SPLIT / RQAMD_PREFILL_TILED switches apply).  All 16-bit operands are
 * bf16, head size = E / nh (64: the register / chunked kernels; anything else up to 256: the plain kernels).
 *
 * One decode step at position t: qkv [rows][3E] (q | k | v of this token), caches kc, vc [rows][nh][Tcap][hd] bf16, y [rows][E].  The
 * token's k / v is appended at cache row t and attends over rows 0 .. t.  ksc != NULL: kc holds bytes with one fp32 scale per cached key
 * in ksc [rows][nh][Tcap], component = (byte - 128) * scale; vsc != NULL (needs ksc): vc likewise.  t_max: the host bound on t that
 * selects the kernel (-1 = Tcap - 1).  step_dev == NULL: t is passed by value; otherwise *step_dev is set to step_base on the stream
 * first and the kernel reads t = *step_dev + (t - step_base), as a captured graph does.  Refused with RQAMD_ERR_INVALID before any launch
 * (the kernels trap on a position outside the host bound): a null qkv or y, rows, nh, E or Tcap < 1, t < 0, t >= Tcap, t_max >= Tcap,
 * 0 <= t_max < t, a missing kc or vc, vsc without ksc.  The launcher's own refusals pass through (RQAMD_ERR_UNSUPPORTED: 8-bit caches
 * with Tcap > 256 or a head size other than 64, head size > 256, a head size other than 64 with Tcap > 256). */
int rqamd_dbg_rqt_attn_decode(const void* qkv, void* kc, void* vc, float* ksc, float* vsc, int rows, int nh, int E, int Tcap, int t,
                              int t_max, int* step_dev, int step_base, void* y, void* stream);
/* The causal attention over a prefix of P tokens per image: qkv [n_img * P][3E], y [n_img * P][E]; the k / v of token i are appended at
 * cache row i of caches laid out as above with rows = n_img (rows P .. Tcap-1 are not touched).  kc == NULL (with vc, ksc, vsc): the
 * cache-free form.  Refused with RQAMD_ERR_INVALID: a null qkv or y, n_img, nh or E < 1, vsc without ksc, kc without vc, the cache-free
 * form with another cache pointer; with RQAMD_ERR_UNSUPPORTED: P < 1, P > Tcap, 8-bit caches with P > 255, and the head-size limits above. */
int rqamd_dbg_rqt_attn_prefill(const void* qkv, void* kc, void* vc, float* ksc, float* vsc, int n_img, int P, int nh, int E, int Tcap,
                               void* y, void* stream);
/* The causal attention of R new tokens per image behind a cache that already holds rows 0 .. T0-1 (csrc/rqt_attn_extend.hip): qkv
 * [n_img * R][3E], y [n_img * R][E], caches kc, vc [n_img][nh][Tcap][64] bf16.  Query r attends over cache rows 0 .. T0-1 and over the own
 * keys 0 .. r of the qkv rows; the k / v of token r are appended at cache row T0 + r.  Rows >= T0 are never read, rows >= T0 + R not
 * touched.  Output and appended rows are bit for bit those of rqamd_dbg_rqt_attn_prefill over all T0 + R tokens.  Refused before any
 * launch with RQAMD_ERR_INVALID: a null pointer, n_img, nh, E, R or T0 < 1, T0 + R > Tcap; with RQAMD_ERR_UNSUPPORTED: a head size other
 * than 64, Tcap > RQAMD_RQT_MAX_CONTEXT.  There are no 8-bit forms. */
int rqamd_dbg_rqt_attn_extend(const void* qkv, void* kc, void* vc, int n_img, int R, int T0, int nh, int E, int Tcap, void* y, void* stream);
/* Causal attention inside groups of `group` consecutive rows (the depth axis of the head stack): qkv [rows][3E] -> y [rows][E].
 * Refused with RQAMD_ERR_INVALID: a null qkv or y, E not a multiple of nh, group outside 1 .. 8, rows not a multiple of group. */
int rqamd_dbg_rqt_attn_packed(const void* qkv, int rows, int group, int nh, int E, void* y, void* stream);
/* The decode attention of shared-prompt sampling alone (csrc/rqt_attn_shared.hip), in the style of rqamd_dbg_rqt_attn_decode.  The `fan`
 * consecutive rows of a group share the read-only caches kc_shared, vc_shared [rows / fan][nh][Ps][64]; the own caches kc, vc are
 * [rows][nh][Tcap_row][64].  Global key j < Ps is the group's row j, key j >= Ps own row j - Ps; this token (global index t) is appended
 * at own row t - Ps and attends over keys 0 .. t.  Output and appended rows are bit for bit those of rqamd_dbg_rqt_attn_decode on caches
 * [rows][nh][Ps + Tcap_row][64] that hold a copy of the group's prefix in front of each row's own positions.  t_max (-1 = Ps + Tcap_row - 1),
 * step_dev and step_base as above.  Refused with
 * RQAMD_ERR_INVALID before any launch: a null pointer, rows, fan, nh, E, Ps or Tcap_row < 1, rows % fan != 0, t < Ps, t - Ps >= Tcap_row,
 * t_max >= Ps + Tcap_row, 0 <= t_max < t; with RQAMD_ERR_UNSUPPORTED: a head size other than 64, Ps + Tcap_row > 256. */
int rqamd_dbg_rqt_attn_shared(const void* qkv, const void* kc_shared, const void* vc_shared, void* kc, void* vc, int rows, int fan, int nh,
                              int E, int Ps, int Tcap_row, int t, int t_max, int* step_dev, int step_base, void* y, void* stream);

/* Kernel variants are selected by the number of rows (batch).  factor > 1 makes the selection logic see rows * factor, so
 * that the large-batch variants run on test-sized inputs (results must not change); 1 restores normal behaviour. */
int rqamd_dbg_set_row_scale(int factor);
/* Diagnostics (scripts/lanes_probe2.py, round 6): `dst` -- a handle of the same configuration that has not run yet -- drops its own
 * parameter arena and runs on `src`'s (its own workspace, KV caches, graphs): two handles fed half a batch each on two streams are two
 * independent decode chains over one copy of the weights.  Measured slower than one chain at every batch (profiles/r06_lanes_probe.txt);
 * not used by the product path. */
int rqamd_dbg_rqt_share_params(rqamd_rqt* dst, const rqamd_rqt* src);

/* The dense bf16 MFMA rate the board sustains, measured: `launches` launches of one 512-thread workgroup per CU, every wavefront issuing
 * n_per_wave v_mfma_f32_32x32x16_bf16 from registers alone.  mode 0: constant operands (the data-sheet instruction rate); mode 1: operands
 * that change with every instruction (~N(0,1) bf16), which the board's power limit lets through at a lower clock.  scratch: >= 4 device
 * bytes; *flop_out = the FLOPs issued (the caller times the stream).  bench.py reports the mode-1 rate beside `roofline.peak`. */
int rqamd_dbg_mfma_rate(int mode, int n_per_wave, int launches, float* scratch, double* flop_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RQAMD_H */
