/*
 * ffmi.h -- C ABI of the MI355X-native SpecInfer hot path (libffmi.so).
 *
 * Drop-in boundary for the reference's Op/OpMeta kernel-wrapper layer
 * (hugolatendresse/FlexFlow @ 2025-01-17).  Each entry point names the
 * reference interface it replaces.  Plain C types only: device pointers,
 * sizes, an explicit hipStream_t.  Activations are caller-owned; KV caches and
 * workspaces are handle-owned (the reference's Meta objects own them too,
 * inc_multihead_self_attention.cu:1621-1807).  No exceptions cross the ABI:
 * every call returns an ffmi_status (the reference asserts instead,
 * cuda_helper.h:40-58; a caller shim may assert on != FFMI_OK).
 *
 * Threading: a handle is used by one host thread at a time, like an OpMeta
 * (one GPU task thread per processor in Legion).  All device work is ordered
 * on the stream argument.
 */
#ifndef FFMI_H_
#define FFMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t *ffmi_stream; /* == hipStream_t */

typedef enum {
  FFMI_OK = 0,
  FFMI_ERR_INVALID = 1,     /* bad argument / shape the kernels do not cover */
  FFMI_ERR_HIP = 2,         /* HIP runtime error */
  FFMI_ERR_NCCL = 3,        /* RCCL error */
  FFMI_ERR_OOM = 4,         /* device allocation failed */
  FFMI_ERR_UNSUPPORTED = 5, /* head size / mode not built */
  FFMI_ERR_NO_DEVICE = 6    /* no gfx950 device visible */
} ffmi_status;

typedef enum { FFMI_F16 = 0, FFMI_F32 = 1, FFMI_I32 = 2 } ffmi_dtype;

/* Attention mode == the reference op that the handle replaces. */
typedef enum {
  FFMI_ATTN_INC = 0,  /* IncMultiHeadSelfAttention     (inc_decoding)  */
  FFMI_ATTN_SPEC = 1, /* SpecIncMultiHeadSelfAttention (SSM beam step) */
  FFMI_ATTN_TREE = 2  /* TreeIncMultiHeadSelfAttention (LLM verify)    */
} ffmi_attn_mode;

/* ------------------------------------------------------------------------ */
/* Device batch metadata                                                     */
/* ------------------------------------------------------------------------ */
/* One packed blob per step replaces the reference's per-step H2D copies of
 * tokensInfo / requestsInfo / causalMask / committed_tokens / beam info
 * (request_manager.cu:23-159, ~83-150 KB per GPU per step): the host packs
 * only what the step uses, in the form the kernels read.                    */

typedef struct {
  int32_t token_id;   /* input token (embedding row)                         */
  int32_t pos;        /* RoPE position = abs_depth_in_request                */
  int32_t req;        /* request slot (KV-cache row)                         */
  int32_t store_slot; /* KV-cache slot this token's K/V goes to (-1: none)   */
  int32_t prefix_len; /* keys [0, prefix_len) are visible to this token      */
  int32_t tree_base;  /* first tree slot                                     */
  int32_t tree_len;   /* tree slots [tree_base, tree_base+tree_len) ...      */
  int32_t tree_bit;   /* ... visible iff mask[req][slot-tree_base] bit set   */
  uint64_t tree_vis;  /* OUTPUT of ffmi_batch_upload (input ignored): the same
                         rule transposed for this query, bit j set iff tree
                         slot tree_base+j is visible -- what kernels read */
} ffmi_token_info;

typedef struct {
  int32_t req;     /* request slot                                         */
  int32_t q_start; /* first batch token of this work item                  */
  int32_t q_count; /* tokens in the item (<= FFMI_ATTN_QTILE)              */
  int32_t kv_len;  /* keys scanned: [0, kv_len)                            */
} ffmi_attn_work;

typedef struct {
  int32_t src_token; /* token index in the PREVIOUS verify batch (staging) */
  int32_t req;       /* request slot                                       */
  int32_t depth;     /* destination KV slot (token depth)                  */
  int32_t pad;
} ffmi_commit_info;

#define FFMI_ATTN_QTILE 32
#define FFMI_MAX_TREE 64

/* Host-side description of one step (pointers into host memory). */
typedef struct {
  int32_t num_tokens;
  int32_t num_work;
  int32_t num_commits;
  int32_t num_mask_reqs;        /* rows in `masks` (indexed by req slot)    */
  const ffmi_token_info *tokens;   /* [num_tokens]                          */
  const ffmi_attn_work *work;      /* [num_work]                            */
  const ffmi_commit_info *commits; /* [num_commits]                         */
  const uint64_t *masks;           /* [num_mask_reqs][FFMI_MAX_TREE]        */
} ffmi_batch_desc;

typedef struct ffmi_batch_dev ffmi_batch_dev; /* device copy + pinned staging */

ffmi_status ffmi_batch_create(int max_tokens, int max_requests, ffmi_batch_dev **out);
void ffmi_batch_destroy(ffmi_batch_dev *b);
/* Replaces RM_LOAD_TOKENS / RM_LOAD_BATCH_CONFIG tasks
 * (request_manager.cu:23-159): one async H2D copy of the used bytes. */
ffmi_status ffmi_batch_upload(ffmi_batch_dev *b, const ffmi_batch_desc *desc,
                              ffmi_stream stream);

/* ------------------------------------------------------------------------ */
/* Attention (replaces src/ops/{inc,spec_inc,tree_inc}_multihead_self_attention) */
/* ------------------------------------------------------------------------ */
typedef struct {
  int mode;            /* ffmi_attn_mode                                     */
  int num_heads;       /* heads on this shard                                */
  int head_dim;        /* 64 or 128; 32 too in FFMI_ATTN_INC (inc...cu:911) */
  int max_requests;    /* KV rows                                            */
  int max_seq_len;     /* committed slots per request (S)                    */
  int max_tree_tokens; /* extra slots for tree / spec (S' = S + tree)        */
  int max_tokens;      /* batch capacity (staging rows for TREE commits)     */
  float qk_scale;      /* 1/sqrt(head_dim) (qk_prod_scaling)                 */
  float rope_theta;    /* HF rotate-half RoPE base                           */
  int out_layout;      /* 0: out [T][heads*head_dim] row-major;
                          1: packed activation tiles (feeds ffmi_linear with
                          FFMI_X_PACKED; heads*head_dim % 32 == 0)          */
  /* llama3 RoPE frequency scaling as HF transformers defines it: the band of
   * a frequency pair from its wavelength 2*pi / inv_freq (the reference's
   * inc_multihead_self_attention.cu:704-722 takes it of pos * inv_freq);
   * rope_llama3 = 0: plain HF RoPE, the other fields ignored               */
  int rope_llama3;
  float rope_factor, rope_low_freq_factor, rope_high_freq_factor;
  int rope_original_max_pos;
  /* 1: DT_FLOAT (--use-full-precision): qkv in and out fp32 row-major
   * (out_layout 0), K and V caches fp32 [req][head][slot][d] both, fp32
   * softmax (kernels/f32.hip).  0: fp16. */
  int full_precision;
} ffmi_attn_cfg;

typedef struct ffmi_attn ffmi_attn;

/* init_task -> IncMultiHeadSelfAttentionMeta ctor (inc_mha.cu:1621-1807) */
ffmi_status ffmi_attn_create(const ffmi_attn_cfg *cfg, ffmi_attn **out);
void ffmi_attn_destroy(ffmi_attn *h);
/* IncMultiHeadSelfAttention::inference_kernel_wrapper (inc_mha.h:115-119) */
ffmi_status ffmi_attn_inc(ffmi_attn *h, const ffmi_batch_dev *b, const void *qkv,
                          void *out, ffmi_stream stream);
/* SpecIncMultiHeadSelfAttention::inference_kernel_wrapper (spec_inc_mha.h:102) */
ffmi_status ffmi_attn_spec(ffmi_attn *h, const ffmi_batch_dev *b, const void *qkv,
                           void *out, ffmi_stream stream);
/* TreeIncMultiHeadSelfAttention::inference_kernel_wrapper (tree_inc_mha.h:104);
 * commits the previous verify batch's accepted K/V first (tree_inc...cu:583-606) */
ffmi_status ffmi_attn_tree(ffmi_attn *h, const ffmi_batch_dev *b, const void *qkv,
                           void *out, ffmi_stream stream);
/* test hooks: raw KV cache pointers and layout ([req][head][slot][d] for K,
 * [req][head][d][slot] for V -- full precision: [req][head][slot][d] for
 * both, fp32 -- slots = max_seq_len + max_tree_tokens rounded up to 32).
 * A GQA handle (ffmi_attn_create_gqa): `head` runs over its num_kv_heads. */
ffmi_status ffmi_attn_kv_ptrs(ffmi_attn *h, void **k, void **v, int *slots);

/* Native grouped-query attention (an extension: the reference replicates each
 * K/V head to its query heads, file_loader.cc:292-302).  Query head h attends
 * K/V head h / G, G = cfg->num_heads / num_kv_heads (HF repeat_kv).  The
 * handle's qkv rows are [num_heads d | num_kv_heads d | num_kv_heads d], its
 * caches K[req][kv_head][slot][d] and V^T[req][kv_head][d][slot], its TREE
 * staging rows 2 num_kv_heads d values; ffmi_attn_inc / _spec / _tree take it
 * as they take any handle (q, out: [T][num_heads d]).  fp16, head_dim 64 / 128.
 * num_kv_heads <= 0 or == num_heads: ffmi_attn_create.  Not a divisor of
 * num_heads: FFMI_ERR_INVALID.  cfg->full_precision (or head_dim 32) with
 * G > 1: FFMI_ERR_UNSUPPORTED ("native gqa" in ffmi_last_error).  These are
 * decided before the device is touched. */
ffmi_status ffmi_attn_create_gqa(const ffmi_attn_cfg *cfg, int num_kv_heads, ffmi_attn **out);
/* bytes of the handle's K plus V caches */
size_t ffmi_attn_cache_bytes(ffmi_attn *h);
/* test and A/B hook of a GQA handle: 0 auto, 1 kv-indexed (one workgroup per
 * item and query head, each reading K/V head h / G), 2 group-shared wherever
 * eligible (one workgroup per item and K/V head, every item's queries x G <=
 * 16).  The routes give the same bits.  No effect on an MHA handle. */
ffmi_status ffmi_attn_set_gqa_route(ffmi_attn *h, int route);

/* ------------------------------------------------------------------------ */
/* Linear (replaces Kernels::Linear::inference_kernel_wrapper,               */
/* linear_kernels.h:54-62; cublasGemmEx at linear_kernels.cu:510-528)        */
/* ------------------------------------------------------------------------ */
typedef enum {
  FFMI_EPI_NONE = 0,    /* Y = X W^T                                           */
  FFMI_EPI_SILU_MUL = 1 /* W = [gate;up] (2N rows): Y = silu(X Wg^T) * (X Wu^T)
                           (fuses SigmoidSiluMulti, sigmoid_silu_multi.cu:37-47) */
} ffmi_epilogue;

/* OR into `epilogue`: X is in packed activation tiles (ffmi_pack_activations)
 * instead of row-major [T][K] -- the operand-fragment order of the weights, so
 * a GEMM reads each activation fragment as one contiguous 1 KiB.  T > 64. */
#define FFMI_X_PACKED 0x10
/* OR into `epilogue`: write Y in packed activation tiles (a GEMM input of the
 * next layer; out_dim % 32 == 0). */
#define FFMI_Y_PACKED 0x20
/* OR into `epilogue`: the weights are a once-read stream (a model larger than
 * the 256 MiB Infinity Cache): their loads carry the non-temporal hint so they
 * do not evict the KV cache, activations or a small model's weights.  Long-K
 * launches of <= 64 rows then split K over 4 waves instead of 8 (faster under
 * the hint): results within the GEMM tolerance of the default policy, and
 * still independent of T within the <= 64-row regime. */
#define FFMI_W_STREAM 0x40
size_t ffmi_packed_activation_bytes(int T, int in_dim);
ffmi_status ffmi_pack_activations(const void *X, int T, int in_dim, void *X_packed,
                                  ffmi_stream stream);

/* Bytes of the MFMA-swizzled weight for an [N][K] fp16 matrix. */
size_t ffmi_linear_packed_bytes(int out_dim, int in_dim);
/* [N][K] row-major fp16 (HF layout) -> MFMA fragment order.  For
 * FFMI_EPI_SILU_MUL pass gate and up separately; they are interleaved. */
ffmi_status ffmi_linear_pack_weight(const void *W, int out_dim, int in_dim,
                                    void *W_packed, ffmi_stream stream);
ffmi_status ffmi_linear_pack_gate_up(const void *Wg, const void *Wu, int out_dim,
                                     int in_dim, void *W_packed, ffmi_stream stream);
/* Y[T][out] = X[T][in] . W^T, fp16 in/out, fp32 accumulate.  Uses a
 * library-owned split-K workspace: calls on different streams must not
 * overlap (use ffmi_linear_ws for that). */
ffmi_status ffmi_linear(const void *X, const void *W_packed, void *Y, int T,
                        int out_dim, int in_dim, int epilogue, ffmi_stream stream);
/* Linear on DT_FLOAT (linear_kernels.cu:450-582 with the full-precision
 * model's fp32 tensors): Y[T][out] = X[T][in] . W[out][in]^T, row-major fp32,
 * exact fp32 arithmetic (v_mfma_f32_16x16x4_f32: an fmaf chain per k range,
 * the k ranges of a workgroup summed in a fixed order).  in_dim % 32 == 0. */
ffmi_status ffmi_linear_f32(const float *X, const float *W, float *Y, int T, int out_dim,
                            int in_dim, ffmi_stream stream);
/* same with a caller-owned workspace of ffmi_linear_workspace_bytes() bytes */
size_t ffmi_linear_workspace_bytes(int T, int out_dim, int in_dim, int epilogue);
ffmi_status ffmi_linear_ws(const void *X, const void *W_packed, void *Y, int T,
                           int out_dim, int in_dim, int epilogue, void *workspace,
                           size_t workspace_bytes, ffmi_stream stream);

/* ------------------------------------------------------------------------ */
/* Norms (replace Kernels::RMSNorm / ResidualRMSNorm inference_kernel_wrapper, */
/* rms_norm_kernels.h:50-54, residual_rms_norm_kernels.h:53-59)              */
/* ------------------------------------------------------------------------ */
ffmi_status ffmi_rmsnorm(const void *x, const void *w, void *out, int T, int H,
                         float eps, ffmi_stream stream);
ffmi_status ffmi_residual_rmsnorm(const void *x1, const void *x2, const void *w,
                                  void *residual_out, void *out, int T, int H,
                                  float eps, ffmi_stream stream);
/* Either norm (x2 == NULL: plain RMSNorm) with flags: FFMI_Y_PACKED writes
 * `out` in packed activation tiles for a following ffmi_linear. */
ffmi_status ffmi_rmsnorm_ex(const void *x1, const void *x2, const void *w, void *residual_out,
                            void *out, int T, int H, float eps, int flags, ffmi_stream stream);

/* ------------------------------------------------------------------------ */
/* Tensor-parallel all-reduce (replaces Kernels::AllReduce::                 */
/* inference_kernel_wrapper, allreduce_kernels.h:28-31 / .cu:53-75)          */
/* ------------------------------------------------------------------------ */
typedef struct ffmi_comm ffmi_comm;
#define FFMI_UNIQUE_ID_BYTES 128
ffmi_status ffmi_comm_unique_id(void *id_out /* FFMI_UNIQUE_ID_BYTES */);
ffmi_status ffmi_comm_create(const void *id, int nranks, int rank, ffmi_comm **out);
/* In-process shard group: `nranks` (<= 8) communicators for host THREADS of
 * one process that step the TP shards of a model on one device (the
 * reference's TP-invariance tests, cpp_inference_tests.sh:203-217, on a
 * single GPU).  out[r] is rank r; destroy each with ffmi_comm_destroy. */
ffmi_status ffmi_comm_create_local(int nranks, ffmi_comm **out);
void ffmi_comm_destroy(ffmi_comm *c);
ffmi_status ffmi_allreduce(ffmi_comm *c, const void *in, void *out, size_t count,
                           int dtype, ffmi_stream stream);

/* Direct xGMI transport (replaces the NCCL data path of the same wrapper,
 * allreduce_kernels.cu:53-75, for a node's ranks).  Every rank exports one
 * exchange buffer of 4 x max_bytes (+ a 20 KiB header) as an IPC handle; the
 * caller's control plane all-gathers the handles ([nranks][64 B], rank
 * order) and every rank attaches them.  ffmi_allreduce on such a
 * communicator then runs ONE kernel per call: copy-in, a flag pushed into
 * each peer's memory, and a one-shot (every rank sums all partials) or
 * two-shot (reduce-scatter + all-gather through the peers' buffers) sum in
 * rank order -- bit-identical on every rank, graph-capturable (the epoch is
 * device-resident), never hanging (a peer silent for FFMI_PEER_TIMEOUT_S,
 * default 10, sets an error that ffmi_comm_peer_status reports).  Attach is
 * collective and ends with a checked self-test all-reduce.
 * ffmi_comm_create_peer makes a communicator with no RCCL state (the
 * transport alone: also what the multi-process tests on one GPU use). */
/* Vocab-parallel greedy / speculative tail (replaces the reference's
 * vocab-sharded lm_head + Combine, model.cc:3392-3419 / combine.cc:200-262,
 * followed by Softmax + ArgMax / ArgTopK, softmax.cu:262-288, argmax.cu:62-100,
 * arg_topk.cu:339-448).  Each rank holds logits [T][Vl] for vocabulary ids
 * [rank*Vl, (rank+1)*Vl); every rank gets the GLOBAL k best ids (k <= 4) and
 * their fp16 softmax probabilities, identical to ffmi_arg_topk on the
 * gathered [T][P*Vl] logits (same max, same float rounding of the same
 * double sum, lowest index among equal fp16 probabilities).  Three
 * exchanges of (P x T x 32 B) records over the communicator; `scratch` holds
 * ffmi_vocab_shard_scratch_bytes(P, T) device bytes. */
size_t ffmi_vocab_shard_scratch_bytes(int nranks, int T);
ffmi_status ffmi_vocab_shard_topk(ffmi_comm *c, const void *logits, int T, int Vl, int k,
                                  int32_t *ids, float *probs, void *scratch, ffmi_stream stream);
/* Vocab-parallel top-p sampling: the do_sample tail (ffmi_sample_topp, below)
 * on the same sharded logits.  Every rank gets, per row, the token and the p
 * that ffmi_sample_topp returns on the gathered [T][P*Vl] logits with the same
 * temperature, topp and u -- the same token, not an approximation: the rule's
 * cumulative masses are integer multiples of 2^-24, so they do not depend on
 * how the vocabulary is split.  The logits are never gathered: five exchanges
 * of per-row records (the max, the sum of the exp terms, a 121-bucket mass
 * histogram, the token counts of one bucket's 128 keys, the owner's id) go
 * over the communicator as sum all-reduces, between six kernel launches.  No
 * exchange exceeds 256 KiB: rows are processed in chunks of 256 / P rows (32
 * at P = 8; FFMI_VSHARD_SAMPLE_CHUNK_ROWS, read per call, lowers it for A/B
 * runs and must be the same on every rank), all phases per chunk.
 * `u` is device memory, one uniform in (0, 1] per row, and MUST hold the same
 * values on every rank: that is the caller's duty (ffmi_sampling_counter is a
 * function of seed, request and position only, so ranks that see the same
 * batch draw alike without an exchange).  ids / probs may be pinned host
 * memory, probs may be NULL.  `scratch` is 16-byte aligned device memory of
 * ffmi_vocab_shard_sample_scratch_bytes(P, T, Vl) bytes (the [T][Vl] fp16 key
 * workspace, per-row state and the exchange records; any contents on entry),
 * one per stream in flight.  Kernel launches and ffmi_allreduce calls on
 * `stream` only: graph-capturable like ffmi_vocab_shard_topk.
 * Decided before any HIP call -- FFMI_ERR_INVALID: a null c / logits / u /
 * ids, T < 0, Vl < 1, temperature <= 0, topp outside (0, 1], a missing or too
 * small scratch; FFMI_ERR_UNSUPPORTED: Vl > 983040, (rank + 1) * Vl > 2^31 - 1.
 * T == 0 is FFMI_OK.  Rows with NaN or +inf logits are outside the contract
 * (any in-range or out-of-range id may come back; nothing faults). */
size_t ffmi_vocab_shard_sample_scratch_bytes(int nranks, int T, int Vl);
ffmi_status ffmi_vocab_shard_sample_topp(ffmi_comm *c, const void *logits, int T, int Vl,
                                         float temperature, float topp, const float *u,
                                         int32_t *ids, float *probs, void *scratch,
                                         size_t scratch_bytes, ffmi_stream stream);

#define FFMI_PEER_HANDLE_BYTES 64
ffmi_status ffmi_comm_create_peer(int nranks, int rank, ffmi_comm **out);
ffmi_status ffmi_comm_peer_export(ffmi_comm *c, size_t max_bytes,
                                  void *handle_out /* FFMI_PEER_HANDLE_BYTES */);
ffmi_status ffmi_comm_peer_attach(ffmi_comm *c, const void *handles /* [nranks][64] */);
/* All-gather of equal-size HOST byte blocks over the communicator (any of its
 * transports): all[r * bytes ...] = rank r's block, on every rank.  Blocking;
 * for control data (the distributed SSMs' results), not the hot path. */
ffmi_status ffmi_comm_allgather(ffmi_comm *c, const void *mine, size_t bytes, void *all);
ffmi_status ffmi_comm_peer_status(ffmi_comm *c);
/* Stop using the transport (RCCL again): for a control plane that saw some
 * rank fail its attach -- every rank must take the same transport. */
ffmi_status ffmi_comm_peer_detach(ffmi_comm *c);
/* All-reduce fused with the residual RMSNorm after it (the reference's
 * AllReduce -> ResidualRMSNorm pair of every TP layer, model.cc:3421-3445,
 * allreduce_kernels.cu:53-75 + residual_rms_norm_kernels.cu:98-131), ONE
 * kernel over an attached xGMI transport: `in` is this rank's f16 partial of
 * columns [col0, H) of the [T][H] sum ([T][H - col0], contiguous); columns
 * [0, col0) of the sum are read from `prev` ([T][H], e.g. an earlier
 * ffmi_allreduce of those columns; NULL when col0 == 0).  Then, as
 * ffmi_rmsnorm_ex(residual, sum, w, residual, out, ..., flags):
 * residual = half(residual + sum) in place and out = RMSNorm(residual) * w
 * (FFMI_Y_PACKED: packed activation tiles) -- bit-identical to the unfused
 * pair.  When the transport takes T*H*2 bytes in two shots (> 2 ranks, above
 * its threshold), rank r normalises only rows [T*r/N, T*(r+1)/N) and gathers
 * every other rank's rows of `out`: `out` is complete on every rank,
 * `residual` is updated on this rank's rows only.  rows_out (optional, [2])
 * receives the updated row range. */
ffmi_status ffmi_allreduce_rmsnorm(ffmi_comm *c, const void *in, int T, int H, int col0,
                                   const void *prev, void *residual, const void *w, float eps,
                                   void *out, int flags, int *rows_out, ffmi_stream stream);

/* ------------------------------------------------------------------------ */
/* Auxiliary ops on the LLaMA greedy path                                    */
/* ------------------------------------------------------------------------ */
/* embed_forward_no_aggr (embedding_kernels.cu:233-244): ids from the batch */
ffmi_status ffmi_embedding(const ffmi_batch_dev *b, const void *table, void *out,
                           int H, ffmi_stream stream);
/* SigmoidSiluMulti standalone (sigmoid_silu_multi.cu:37-47) */
ffmi_status ffmi_silu_mul(const void *a, const void *b, void *out, size_t n,
                          ffmi_stream stream);
/* softmax (fp16 output, softmax.cu:262-288) + ArgMax (argmax.cu:62-100):
 * ids[t] = lowest index of max fp16(softmax(logits[t]))               */
ffmi_status ffmi_argmax(const void *logits, int T, int V, int32_t *ids,
                        float *probs, ffmi_stream stream);
/* softmax + ArgTopK (arg_topk.cu:339-448), k <= 4, sorted, lower index on ties */
ffmi_status ffmi_arg_topk(const void *logits, int T, int V, int k, int32_t *ids,
                          float *probs, ffmi_stream stream);
/* the same with a device workspace: rows of a small batch (the SSM's beam
 * steps, decode) are split over several workgroups that each sum 1/G of the
 * row's exp terms, identical results.  `workspace` holds
 * ffmi_arg_topk_workspace_bytes(T) bytes, zero-filled by the caller once
 * (the call leaves it zeroed); one workspace per stream in flight.  NULL or
 * too small: the one-workgroup-per-row form (ffmi_arg_topk). */
size_t ffmi_arg_topk_workspace_bytes(int T);
ffmi_status ffmi_arg_topk_ws(const void *logits, int T, int V, int k, int32_t *ids,
                             float *probs, void *workspace, size_t workspace_bytes,
                             ffmi_stream stream);
/* Top-p sampling, the do_sample tail of the reference's LLaMA graph
 * (llama.cc:286-289: scalar_truediv -> softmax -> sampling.cu).  Per row,
 * with R16 = round-to-nearest-even to fp16:
 *   z_i = R16(float(x_i) / float(R16(temperature)))
 *   p_i = the probability ffmi_arg_topk defines on z (fp16 softmax)
 *   order the tokens by p descending, index ascending among equal p, and pick
 *   the first whose cumulative p reaches t = (double(u) * topp) * topp; if
 *   none does, the last token of the order.
 * ids[t] is the pick, probs[t] (may be NULL) its p.  The threshold is the
 * reference's (sampling.cu:81,99-100 compares prefix / topp >= u * topp, so
 * topp = 0.8 draws from the top 0.64 of the mass); the cumulative sums are
 * exact (integer multiples of 2^-24) and compared in fp64.  `u` is device
 * memory, one uniform in (0, 1] per row; the caller draws it
 * (ffmi_sampling_counter gives a reproducible one).  One launch,
 * graph-capturable; ids / probs may be pinned host memory.  `workspace`
 * holds ffmi_sample_topp_workspace_bytes(T, V) bytes of device memory (any
 * contents), one per stream in flight.  V <= 983040.
 * FFMI_ERR_INVALID: T < 0, V < 1, a null logits / u / ids pointer, a missing
 * or too small workspace, temperature <= 0, topp outside (0, 1]. */
size_t ffmi_sample_topp_workspace_bytes(int T, int V);
ffmi_status ffmi_sample_topp(const void *logits, int T, int V, float temperature, float topp,
                             const float *u, int32_t *ids, float *probs, void *workspace,
                             size_t workspace_bytes, ffmi_stream stream);
/* The sampling draw of a request's token (host only, no device): with
 *   x = seed ^ (uint64(guid) * 0x9e3779b97f4a7c15) ^ (uint64(pos) * 0xd1342543de82ef95)
 * the top 24 bits of the splitmix64 finaliser
 *   x += 0x9e3779b97f4a7c15; x = (x ^ x >> 30) * 0xbf58476d1ce4e5b9;
 *   x = (x ^ x >> 27) * 0x94d049bb133111eb; x ^= x >> 31
 * u = (counter + 1) * 2^-24 lies in (0, 1].  `pos` is the index of the token
 * being produced in the request's token sequence (prompt with BOS, then the
 * generated tokens), so a draw depends on the seed, the request and the
 * position only -- not on the batch around it, the prefill chunking or graph
 * replay. */
uint32_t ffmi_sampling_counter(uint64_t seed, int64_t guid, int pos);
/* Per-token log-probabilities: the log of the full softmax of a row at one
 * scored id s (no top-p cut: under sampling it is the distribution at the
 * temperature, not the truncated one).  With R16 as above,
 *   z_i = x_i                                       (temperature == 0)
 *   z_i = R16(float(x_i) / float(R16(temperature))) (temperature > 0: the row
 *                                                    ffmi_sample_topp sees)
 *   M   = max_i z_i
 *   S   = sum_i exp(float(z_i) - M)                 fp32
 *   lp  = (float(z_s) - M) - log(S)                 fp32, in this order
 * ((z_s - M) first: M + log S first cancels everything at large logits).
 * Row t scores targets[t] when it is >= 0 and picks[t] otherwise; targets ==
 * NULL scores every row's pick.  picks is the ids output of the pick kernel
 * earlier on the same stream (ids in [0, V)); an id outside [0, V) writes a
 * quiet NaN for its row and reads no logit.  lp <= 0, and lp == 0 for V == 1.
 * A row's bits depend on the row, the temperature and the id only -- not on T,
 * the row's index or the launch shape: the row is cut into chunks of 4096
 * logits, every chunk reduced the same way by one workgroup to (m, s), and the
 * chunks' pairs combined in chunk order (no float atomics).  Two launches,
 * graph-capturable; logprobs (and picks) may be pinned host memory.
 * `workspace` holds ffmi_token_logprobs_workspace_bytes(T, V) bytes of device
 * memory (any contents), one per stream in flight.  Decided before any HIP
 * call -- FFMI_ERR_INVALID: T < 0, V < 1, a null logits / logprobs, a null
 * picks while targets is null, a temperature that is negative or not finite,
 * a missing or short workspace; FFMI_ERR_UNSUPPORTED: V > 983040.  T == 0:
 * FFMI_OK, nothing launched. */
size_t ffmi_token_logprobs_workspace_bytes(int T, int V);
ffmi_status ffmi_token_logprobs(const void *logits, int T, int V, float temperature,
                                const int32_t *targets, const int32_t *picks, float *logprobs,
                                void *workspace, size_t workspace_bytes, ffmi_stream stream);
/* DT_FLOAT twins (--use-full-precision, kernels/f32.hip): RMSNorm /
 * ResidualRMSNorm (sum of squares in fp64, rounded once; fp32 residual add),
 * SigmoidSiluMulti, softmax + arg-top-k on fp32 probabilities (k <= 4, lowest
 * index among equal probabilities; k = 1 is the argmax) */
ffmi_status ffmi_rmsnorm_f32(const float *x, const float *w, float *out, int T, int H, float eps,
                             ffmi_stream stream);
ffmi_status ffmi_residual_rmsnorm_f32(const float *x1, const float *x2, const float *w,
                                      float *residual_out, float *out, int T, int H, float eps,
                                      ffmi_stream stream);
ffmi_status ffmi_silu_mul_f32(const float *a, const float *b, float *out, size_t n,
                              ffmi_stream stream);
ffmi_status ffmi_arg_topk_f32(const float *logits, int T, int V, int k, int32_t *ids,
                              float *probs, ffmi_stream stream);
/* seeded synthetic weights, identical to oracle/orc_gen_weight then fp16.
 * kind 0: matrix (uniform, std 0.02); 1: norm weight (1 +- 0.1);
 * FFMI_WKIND_DEPTH | L: o_proj / down_proj of an L-layer model under the
 * depth-scaled init (std 0.02 / sqrt(2L)) */
#define FFMI_WKIND_DEPTH 0x10000
ffmi_status ffmi_fill_weight(void *dst_f16, size_t n, const char *name,
                             uint64_t seed, int kind, ffmi_stream stream);

/* ------------------------------------------------------------------------ */
/* Serving runtime (C++ host side above the kernels; RequestManager API)     */
/* ------------------------------------------------------------------------ */
typedef struct {
  int num_layers, vocab_size, num_heads, num_kv_heads, hidden, intermediate;
  float rms_eps, rope_theta;
  /* llama3 RoPE scaling (llama.h:53-65), as in ffmi_attn_cfg */
  int rope_llama3;
  float rope_factor, rope_low_freq_factor, rope_high_freq_factor;
  int rope_original_max_pos;
} ffmi_llama_config;

typedef enum {
  FFMI_MODEL_INC = 0,  /* INC_DECODING_MODE  */
  FFMI_MODEL_BEAM = 1, /* BEAM_SEARCH_MODE (SSM) */
  FFMI_MODEL_TREE = 2  /* TREE_VERIFY_MODE (LLM) */
} ffmi_model_mode;

typedef struct {
  int mode;                  /* ffmi_model_mode                                */
  int tp_rank, tp_size;      /* tensor parallelism (heads / FFN columns)       */
  ffmi_comm *comm;           /* communicator of tp_size ranks: RCCL, xGMI
                              * transport or local group (NULL when tp_size == 1).
                              * A ONE-rank communicator without RCCL state or
                              * transport with tp_size > 1 runs shard tp_rank
                              * alone, every all-reduce the identity: the
                              * per-rank compute measurement of
                              * scripts/tp_shard_bench.py (tokens meaningless) */
  int max_requests;          /* max_requests_per_batch                         */
  int max_tokens;            /* max tokens per batch (verify capacity for TREE) */
  int max_seq_len;           /* max_sequence_length                            */
  int max_tree_tokens;       /* max_spec_tree_token_num                        */
  uint64_t weight_seed;      /* synthetic weights (orc_gen_weight spec)        */
  int use_graphs;            /* capture per-shape hipGraphs (0/1)              */
  /* Checkpoint in the reference's format (file_loader.cc:217-361,
   * serve/models/llama.py convert_hf_model): one raw fp16 or fp32 file per
   * tensor, named as the HF parameter without "model." ("embed_tokens.weight",
   * "layers.0.self_attn.q_proj.weight", ..., "norm.weight", "lm_head.weight").
   * K/V projections of GQA checkpoints are replicated to every query head as
   * the reference does (file_loader.cc:292-302), unless the model is created
   * with FFMI_MODEL_NATIVE_GQA (ffmi_model_create_ex).  NULL: synthetic weights. */
  const char *weights_folder;
  /* synthetic weights (no weights_folder), oracle.h orc_model_create_ex:
   * 0: every matrix uniform with std 0.02 (the bench's model);
   * 1: depth-scaled -- o_proj / down_proj at std 0.02 / sqrt(2L);
   * 2: token chain -- embeddings x 128 (x 2 per doubling of the residual
   *    noise sqrt(L (H + 2F)) over LLaMA-7B's; 65B: x 512) and lm_head = the
   *    embedding rows permuted (v -> (7919 v + 17) mod vocab): a peaked model whose greedy
   *    picks lead by margins far above fp16 rounding noise (parity tests of
   *    the reference's literal token bars; SpecInfer with full acceptance) */
  int weight_init;
  /* 1: full precision -- the reference's --use-full-precision
   * (spec_infer.cc:102, incr_decoding.cc:77): weights, activations, KV cache
   * and softmax in fp32 (runtime/llama_f32.cpp, kernels/f32.hip); lm_head
   * replicated under TP.  0: the fp16 model (the measured path). */
  int full_precision;
} ffmi_model_opts;

typedef struct ffmi_model ffmi_model;
ffmi_status ffmi_model_create(const ffmi_llama_config *cfg, const ffmi_model_opts *o,
                              ffmi_model **out);
/* flags: FFMI_MODEL_* bits; 0 is ffmi_model_create.
 *   FFMI_MODEL_NATIVE_GQA: K/V projections, the qkv GEMM and the KV cache at
 *   num_key_value_heads (ffmi_attn_create_gqa) instead of replicated to every
 *   query head: wqkv has (num_heads + 2 num_kv_heads) d / tp_size rows per
 *   rank, each rank its own K/V heads.  fp16 only (full_precision:
 *   FFMI_ERR_UNSUPPORTED); num_kv_heads % tp_size != 0: FFMI_ERR_UNSUPPORTED
 *   ("native_gqa" in ffmi_last_error) -- the replicated load takes that case.
 *   Synthetic weights may have num_kv_heads < num_heads under the flag. */
#define FFMI_MODEL_NATIVE_GQA 1u
ffmi_status ffmi_model_create_ex(const ffmi_llama_config *cfg, const ffmi_model_opts *o,
                                 unsigned flags, ffmi_model **out);
/*   FFMI_MODEL_LORA: the model serves LoRA adapters on the attention
 *   projections q_proj, k_proj, v_proj, o_proj and on down_proj (the
 *   reference's LoraLinear, lora_linear.cc; gate_proj / up_proj are not
 *   served), one adapter per request at most, requests of different adapters
 *   and of none in one batch.  fp16 INC and TREE models at tp_size 1 only:
 *   BEAM (SSMs run without adapters), full_precision and tp_size > 1 return
 *   FFMI_ERR_UNSUPPORTED ("lora" in ffmi_last_error).  A step's module mask is
 *   the union of the modules of the adapters its rows name; a row without an
 *   adapter keeps the bits it has in a step without adapters.  The route of
 *   each module in the mask:
 *     q / k / v: the attention norm runs as a launch, the qkv GEMM rounds its
 *       split-K sums to fp16 [T][Nqkv] and ffmi_lora_apply_qkv follows on
 *       that row, ahead of RoPE and the KV store (FFMI_DBG_QKV then holds the
 *       adapted row);
 *     o: where the o projection is folded into the attention it stays there
 *       (its per-head slabs are then summed in head order and rounded once,
 *       the value the residual norm computes from them); otherwise the o GEMM
 *       runs outside the fused residual norms, its split-K sums rounded to
 *       fp16 [T][H].  ffmi_lora_apply follows on that with x the attention
 *       output, then the residual norm as a launch (FFMI_DBG_O_PROJ: adapted);
 *     down: down_proj runs outside the fused residual norms, its split-K sums
 *       are rounded to fp16 [T][H] and ffmi_lora_apply follows on that
 *       (FFMI_DBG_DOWN then holds the adapted output).
 *   A step with an empty mask is the step of a model without the flag, launch
 *   for launch, with one exception: the fused residual norms are not
 *   bit-identical to the norm launches, so on a model that uses them (hidden
 *   >= 2048 by default, FFMI_FUSE_NORM) the route is decided at load time --
 *   while an adapter with an attention module (q, k, v, o) is resident, every
 *   step takes the routes above of all of that adapter's modules, whatever
 *   its rows name.  (A down-only adapter keeps its per-step route: a step
 *   that names none is the fused step.) */
/*   (bit value 4: 2 stays an unknown flag, FFMI_ERR_INVALID, as it was before
 *   the adapters came and as callers written against that may rely on) */
#define FFMI_MODEL_LORA 4u
/* LoRA adapters of a FFMI_MODEL_LORA model.  Adapter ids are process-wide
 * (0 .. FFMI_LORA_MAX_ADAPTERS - 1): a request names one at registration
 * (ffmi_rm_register_request_ex) and the model that loaded it serves it.
 *   load: A [L][rank][F] and B [L][H][rank] fp16 host arrays, row-major as
 *   HF PEFT stores lora_A.weight / lora_B.weight of every layer's down_proj;
 *   scaling = fp16(alpha / rank).  1 <= rank <= FFMI_LORA_MAX_RANK (stored
 *   zero-padded); a larger rank: FFMI_ERR_UNSUPPORTED ("lora").  No free id:
 *   FFMI_ERR_OOM.  Device storage is allocated here, never in a step.  The
 *   one-module (down) case of load_modules.
 *   load_modules: n modules of one adapter, each once, one rank and one alpha
 *   for all (PEFT's rank_pattern is not served).  A [L][rank][in] and B
 *   [L][out][rank] fp16 host arrays in the HF shapes: q (in H, out H), k and v
 *   (H, num_kv_heads * head_dim), o (H, H), down (F, H).  Under the default
 *   replicated load of a GQA checkpoint the rows of a k / v B are replicated
 *   to the query heads as the loader replicates the k / v weights (query head
 *   h uses K/V head h / G); under FFMI_MODEL_NATIVE_GQA they are taken as
 *   stored.  n == 0, a module twice or an unknown module id: FFMI_ERR_INVALID;
 *   FFMI_LORA_GATE / FFMI_LORA_UP: FFMI_ERR_UNSUPPORTED (their GEMM's SiLU-mul
 *   epilogue never leaves the pre-activation values in memory); "lora" in
 *   ffmi_last_error in both cases.
 *   load_folder: the reference's per-tensor files
 *   layers.{i}.mlp.down_proj.lora_A.weight / .lora_B.weight in `folder`
 *   (peft_weight_allocator.cc:171-240), fp16 or fp32 by file size.  A file of
 *   another target module in the folder (q_proj, up_proj, ...):
 *   FFMI_ERR_UNSUPPORTED ("lora").  The modules == FFMI_LORA_DOWN_BIT case of
 *   load_folder_ex.
 *   load_folder_ex: layers.{i}.self_attn.{q,k,v,o}_proj.lora_{A,B}.weight and
 *   layers.{i}.mlp.down_proj.lora_{A,B}.weight of the modules in the mask
 *   `modules` (FFMI_LORA_*_BIT).  FFMI_ERR_UNSUPPORTED ("lora"): a .lora_ file
 *   of a module outside the mask or of gate_proj / up_proj in the folder, a
 *   file of a module in the mask missing or of the wrong size.
 *   unload: FFMI_ERR_INVALID while a registered, unfinished request names the
 *   adapter, or for an id this model did not load; frees every module. */
#define FFMI_LORA_MAX_ADAPTERS 8
#define FFMI_LORA_MAX_RANK 64
ffmi_status ffmi_model_lora_load(ffmi_model *m, int rank, float alpha, const void *A,
                                 const void *B, int *id_out);
ffmi_status ffmi_model_lora_load_folder(ffmi_model *m, const char *folder, int rank, float alpha,
                                        int *id_out);
ffmi_status ffmi_model_lora_unload(ffmi_model *m, int id);
/* module ids of an adapter and their bit masks (1u << id) */
#define FFMI_LORA_Q 0
#define FFMI_LORA_K 1
#define FFMI_LORA_V 2
#define FFMI_LORA_O 3
#define FFMI_LORA_DOWN 4
#define FFMI_LORA_GATE 5 /* refused */
#define FFMI_LORA_UP 6   /* refused */
#define FFMI_LORA_Q_BIT (1u << FFMI_LORA_Q)
#define FFMI_LORA_K_BIT (1u << FFMI_LORA_K)
#define FFMI_LORA_V_BIT (1u << FFMI_LORA_V)
#define FFMI_LORA_O_BIT (1u << FFMI_LORA_O)
#define FFMI_LORA_DOWN_BIT (1u << FFMI_LORA_DOWN)
typedef struct {
  int module; /* FFMI_LORA_Q .. FFMI_LORA_DOWN */
  const void *A, *B;
} ffmi_lora_module;
ffmi_status ffmi_model_lora_load_modules(ffmi_model *m, int rank, float alpha, int n,
                                         const ffmi_lora_module *mods, int *id_out);
ffmi_status ffmi_model_lora_load_folder_ex(ffmi_model *m, const char *folder, int rank,
                                           float alpha, unsigned modules, int *id_out);
/* The LoRA update of a [T][H] fp16 projection output, in place:
 *   h[t][j]  = fp16(sum_k x[t][k] A[j][k])            (fp32 accumulation)
 *   y[t][n]  = fp16(float(y[t][n]) + scale * sum_j h[t][j] B[n][j])
 * for every row t with 0 <= slots[t] < FFMI_LORA_MAX_ADAPTERS and a non-NULL
 * table entry; other rows of y are not written.  A row's result depends on
 * the row, its adapter and F only (F is split in 256-column parts whose fp32
 * partial sums are added in part order), not on T or the rows around it.
 *   x: [T][F] fp16 row-major, or packed activation tiles (x_packed != 0;
 *   ffmi_pack_activations).  slots: [T] int32 on the device.  table:
 *   FFMI_LORA_MAX_ADAPTERS device-resident ffmi_lora_entry; A packed as
 *   ffmi_pack_activations packs a [64][F] matrix (rows >= rank zero), B
 *   [H][64] row-major (columns >= rank zero), scale = float(fp16(alpha / r)).
 *   ws: ffmi_lora_workspace_bytes(T, F) bytes of device scratch.
 *   h_out: NULL, or [T][64] fp16 (rows with an adapter are written: the
 *   kernel's own h, zero beyond the adapter's rank rounded up to 16).
 * FFMI_ERR_INVALID: F % 32, H % 8, a missing or short workspace. */
typedef struct {
  const void *A, *B;
  float scale;
  int rank;
} ffmi_lora_entry;
size_t ffmi_lora_workspace_bytes(int T, int F);
ffmi_status ffmi_lora_apply(const void *x, int T, int F, int H, const int32_t *slots,
                            const ffmi_lora_entry *table, void *y, int x_packed, void *ws,
                            size_t ws_bytes, void *h_out, ffmi_stream stream);
/* The same update of the fused qkv row y [T][ldy] = [Q | K | V], the segments
 * seg_width[0..2] columns wide, from one x [T][in_dim] (the attention norm's
 * output), in two launches for the three modules.  table[s]: the
 * FFMI_LORA_MAX_ADAPTERS device-resident entries of segment s (A packed from
 * [64][in_dim], B [seg_width[s]][64]); an entry with NULL A or B: the adapter
 * has no such module, and the row's columns of that segment are not written.
 * A row's bits depend on the row, its adapter and the module's dimensions
 * only: not on T, the rows around it or which other segments are present, and
 * they are those of ffmi_lora_apply(x, T, in_dim, seg_width[s]) on the
 * segment alone.  Columns [sum of the widths, ldy) are not touched.
 *   ws: ffmi_lora_qkv_workspace_bytes(T, in_dim) = 3 * ceil(in_dim / 256) * T
 *   * 64 floats.  h_out: NULL, or [3][T][64] fp16, written where the row's
 *   adapter has the segment's module.
 * FFMI_ERR_INVALID: in_dim % 32, a width that is not a positive multiple of 8,
 * ldy below the sum of the widths, a missing or short workspace. */
size_t ffmi_lora_qkv_workspace_bytes(int T, int in_dim);
ffmi_status ffmi_lora_apply_qkv(const void *x, int T, int in_dim, const int *seg_width,
                                const int32_t *slots, const ffmi_lora_entry *const *table,
                                void *y, int ldy, int x_packed, void *ws, size_t ws_bytes,
                                void *h_out, ffmi_stream stream);
/* bytes of the K plus V caches of all layers (this rank's; fp16 models) */
size_t ffmi_model_kv_cache_bytes(ffmi_model *m);
void ffmi_model_destroy(ffmi_model *m);
/* Per-op device timing with HIP events on the model's stream (the
 * reference's --profiling, model.cc:4548-4550).  level 0: off; 1: sampled
 * (layers 0 and L/2 of every 4th step with <= 256 tokens -- FFMI_PROF_EVERY
 * sets the stride; sampled steps run eager, the others replay graphs);
 * 2: every op of every step. */
typedef struct {
  char name[32];
  long launches;
  double total_ms;
  double bytes; /* algorithmic bytes (weights + activations read/written)  */
  double flops;
} ffmi_op_stat;
ffmi_status ffmi_model_set_profiling(ffmi_model *m, int level);
int ffmi_model_op_stats(ffmi_model *m, ffmi_op_stat *out, int cap);
/* Tensor capture for alignment checks (the reference's --inference-debugging
 * per-layer dumps, operator.h:271-360, compared by
 * tests/inference/inference_alignment_test.py).  While enabled, steps run
 * eager (no graph replay) and the LAST step's tensors are kept on the device:
 *   FFMI_DBG_HIDDEN, layer l in [0, num_layers): the residual stream after
 *     decoder layer l (HF hidden_states[l + 1]); layer == num_layers: the
 *     final RMSNorm output (HF's last hidden state);
 *   FFMI_DBG_LOGITS: the lm_head output [T][V_l] (before softmax; V_l = this
 *     rank's vocab shard when the lm_head is vocab-sharded, else vocab);
 * and per op of decoder layer l, the tensors the reference's alignment test
 * compares (inference_alignment_test.py:20-370: embedding, the two norms,
 * the QKV projection with its shard re-assembly, attention output, MLP):
 *   FFMI_DBG_EMBED      [T][H]     embedding rows (layer 0 only)
 *   FFMI_DBG_ATTN_NORM  [T][H]     input_layernorm output
 *   FFMI_DBG_QKV        [T][3*H_l] qkv_proj output before RoPE, [Q_s|K_s|V_s]
 *   FFMI_DBG_ATTN_OUT   [T][H_l]   attention output (o_proj input)
 *   FFMI_DBG_O_PROJ     [T][H]     o_proj output (after the all-reduce)
 *   FFMI_DBG_FFN_NORM   [T][H]     post_attention_layernorm output
 *   FFMI_DBG_MLP_ACT    [T][F_l]   SiLU(gate) * up (down_proj input)
 *   FFMI_DBG_DOWN       [T][H]     down_proj output (after the all-reduce)
 * H_l / F_l are this rank's shard widths.  ffmi_model_debug_tensor copies one
 * as fp32 rows [T][width] into `out` (capacity `cap` floats) and returns T,
 * or -1 (nothing captured / bad argument / too small);
 * ffmi_model_debug_width returns the width (or -1). */
#define FFMI_DBG_HIDDEN 0
#define FFMI_DBG_LOGITS 1
#define FFMI_DBG_ATTN_NORM 2
#define FFMI_DBG_QKV 3
#define FFMI_DBG_ATTN_OUT 4
#define FFMI_DBG_O_PROJ 5
#define FFMI_DBG_FFN_NORM 6
#define FFMI_DBG_MLP_ACT 7
#define FFMI_DBG_DOWN 8
#define FFMI_DBG_EMBED 9
ffmi_status ffmi_model_set_debug(ffmi_model *m, int enable);
/* GenerationConfig(do_sample, temperature, topp) of the reference
 * (inference.h:22-33, llama.cc:284-295).  do_sample != 0: an incremental-
 * decoding model picks every token with ffmi_sample_topp instead of the
 * argmax, u = (ffmi_sampling_counter(seed, request guid, position) + 1) *
 * 2^-24.  A tensor-parallel model with a vocab-sharded lm_head takes
 * ffmi_vocab_shard_sample_topp over its communicator: the same tokens on
 * every rank (each rank draws the same u from the same batch), the steps
 * still replayed as graphs.  temperature <= 0 becomes 0.8 and topp <= 0
 * becomes 0.6, as the reference's constructor; topp > 1 is FFMI_ERR_INVALID.
 * do_sample == 0 restores the greedy tail.  FFMI_ERR_UNSUPPORTED (message in
 * ffmi_last_error) for a BEAM or TREE model (a sampled pick cannot verify a
 * greedy token tree) and a full_precision model. */
ffmi_status ffmi_model_set_sampling(ffmi_model *m, int do_sample, float temperature, float topp,
                                    uint64_t seed);
/* enable != 0: every step of an fp16 INC or TREE model also runs
 * ffmi_token_logprobs behind its pick, in the same stream and captured graph
 * (temperature: the model's when it samples, 0 otherwise), and its results
 * carry one log-probability per row; a serve call with such an LLM records
 * them per request (ffmi_rm_get_logprobs).  Off (the default): no launch and
 * no byte is added to a step.  Toggling synchronises the stream and drops the
 * captured graphs.  FFMI_ERR_UNSUPPORTED ("logprobs" in ffmi_last_error): a
 * BEAM model (an SSM's picks are proposals), a full_precision model, a
 * vocab-sharded lm_head (tensor parallelism over the vocabulary). */
ffmi_status ffmi_model_set_logprobs(ffmi_model *m, int enable);
long ffmi_model_debug_tensor(ffmi_model *m, int which, int layer, float *out, long cap);
long ffmi_model_debug_width(ffmi_model *m, int which);
/* Negative-control fault injection (tests only; never set in serving): the
 * parity tests must FAIL on a model with a deliberate bug.
 *   FFMI_FAULT_ROPE_POS, layer, arg: that layer's RoPE rotates tokens at
 *     positions >= arg by position + 1 (an off-by-one position in one layer's
 *     decode phase, apply_rotary_embedding_hf inc_multihead_self_attention.cu:
 *     664-738 with a wrong abs_depth); layer -1: every layer; arg < 0
 *     clears it.
 *   FFMI_FAULT_RESID_ROUND (layer, arg ignored; fp16 models, process-wide):
 *     the residual RMSNorm kernel squares the UNROUNDED fp32 residual sum
 *     x1 + x2 where residual_rms_norm_kernels.cu:112-114 rounds it to half
 *     first -- a rounding-point bug that moves the normalised outputs by at
 *     most an ulp (the norms folded into the decode GEMMs are not faulted).
 *   FFMI_FAULT_TP_HEAD_SWAP (layer; -1: every layer; fp16 models): this
 *     model's qkv weights with the Q rows of its local heads 0 and 1
 *     exchanged -- a head-offset bug in one rank's shard (file_loader.cc:
 *     286-303 places head h's rows at h * head_dim of the rank's block).
 *   FFMI_FAULT_TP_AR_DROP (layer, arg: 0 = the all-reduce after o_proj, 1 =
 *     after down_proj; TP > 1, fp16 models): this rank's contribution to that
 *     all-reduce is zeroed (a partial sum lost, allreduce.cc:291-331).
 *   FFMI_FAULT_NONE clears every fault. */
#define FFMI_FAULT_NONE 0
#define FFMI_FAULT_ROPE_POS 1
#define FFMI_FAULT_RESID_ROUND 2
#define FFMI_FAULT_TP_HEAD_SWAP 3
#define FFMI_FAULT_TP_AR_DROP 4
ffmi_status ffmi_model_debug_fault(ffmi_model *m, int kind, int layer, int arg);
/* select the HIP device of the calling thread (one process per GPU) */
ffmi_status ffmi_set_device(int device);

typedef struct ffmi_rm ffmi_rm;
typedef struct {
  int max_requests_per_batch;
  int max_tokens_per_batch;
  int max_spec_tree_token_num;
  int max_sequence_length;
  int bos_token_id;        /* <0: none                                       */
  const int *eos_token_ids;
  int num_eos;
  const int *spec_tree_width; /* push_spec_infer_tree_width sequence         */
  int num_tree_width;
  int verbose;
  int spec_extensions;     /* FFMI_SPEC_EXT_* bits (ABI 0.3); 0: the reference's limits */
} ffmi_rm_config;
/* Flagged SpecInfer extensions beyond what the reference runs (BASELINE
 * configs C "tree width=4" and E "4x SSMs"):
 *   FFMI_SPEC_EXT_WIDTH4: tree widths and branches per layer up to 4 (the
 *     reference's MAX_BEAM_WIDTH / MAX_SPECULATIVE_TREE_BRANCHES are 3,
 *     batch_config.h:196,200, request_manager.cc:168-171); size
 *     max_spec_tree_token_num for the tree (27 tokens for widths (1,1,4));
 *   FFMI_SPEC_EXT_MULTI_SSM: more than one registered SSM; their token trees
 *     are united by path (merge_dfs_trees, request_manager.cc:2817-2878, whose
 *     reference form asserts a single SSM) and cut to max_spec_tree_token_num
 *     (<= 64) nodes in layer order. */
#define FFMI_SPEC_EXT_WIDTH4 1
#define FFMI_SPEC_EXT_MULTI_SSM 2

ffmi_status ffmi_rm_create(const ffmi_rm_config *cfg, ffmi_rm **out);
void ffmi_rm_destroy(ffmi_rm *rm);
ffmi_status ffmi_rm_register_ssm(ffmi_rm *rm, ffmi_model *ssm);
/* Config E's SSMs placed over the ranks of a TP group (the reference builds
 * each SSM as its own TP = 1 model, spec_infer.cc:381-435): SSM s runs on
 * rank s % nranks only.  Every rank registers the SSMs in the same order --
 * its own with ffmi_rm_register_ssm, the others with
 * ffmi_rm_register_remote_ssm -- and sets an exchange.  After its SSMs' beam
 * steps a rank contributes their per-step results and replays the other
 * ranks' SSMs' bookkeeping on theirs, so every rank merges the identical token
 * trees (FFMI_SPEC_EXT_MULTI_SSM).  The exchange is an all-gather of equal-
 * size host byte blocks, fn(ctx, mine, bytes, all[nranks][bytes]) returning
 * 0 on success; ffmi_rm_set_ssm_exchange_comm uses ffmi_comm_allgather. */
typedef int (*ffmi_allgather_fn)(void *ctx, const void *mine, size_t bytes, void *all);
ffmi_status ffmi_rm_register_remote_ssm(ffmi_rm *rm);
ffmi_status ffmi_rm_set_ssm_exchange(ffmi_rm *rm, int nranks, int rank, ffmi_allgather_fn fn,
                                     void *ctx);
ffmi_status ffmi_rm_set_ssm_exchange_comm(ffmi_rm *rm, ffmi_comm *comm);
/* RequestManager::register_output_filepath (request_manager.cc:246-249):
 * each completed request is appended in the reference's record format
 * (incr decoding :813-840, SpecInfer :1303-1330).  NULL or "" turns it off. */
ffmi_status ffmi_rm_register_output_filepath(ffmi_rm *rm, const char *path);
/* The text written after "token IDs:" is the reference's
 * tokenizer_->Decode(tokens) (request_manager.cc:786-789): the runtime calls
 * fn(ids, n, NULL, 0, ctx) for the byte length, then fn(ids, n, buf, len, ctx).
 * NULL fn: empty text (no tokenizer). */
typedef int (*ffmi_detokenize_fn)(const int *ids, int n, char *buf, int cap, void *ctx);
ffmi_status ffmi_rm_register_detokenizer(ffmi_rm *rm, ffmi_detokenize_fn fn, void *ctx);
/* The tokenizer is the old LLaMA SentencePiece model (the reference's
 * old_llama_tokenizer, request_manager.cc:200-211): SentencePiece drops BOS
 * when decoding, so the text of a request registered with
 * add_special_tokens whose tokens start with BOS gets a "<s> " prefix
 * (:776-781). */
ffmi_status ffmi_rm_set_old_llama_tokenizer(ffmi_rm *rm, int enable);
/* Request: prompt token ids (BOS is prepended when bos_token_id >= 0 and
 * add_special_tokens), max_length / max_new_tokens as in Request
 * (request_manager.cc:334-441).  Returns guid (> 0) or 0 on rejection. */
int64_t ffmi_rm_register_request(ffmi_rm *rm, const int *prompt, int n_prompt,
                                 int max_length, int max_new_tokens,
                                 int add_special_tokens);
/* The same with a LoRA adapter: lora_id -1 (none; ffmi_rm_register_request)
 * or the id of a loaded adapter (ffmi_model_lora_load), which every LLM step
 * of the request applies; SSM steps run without it.  An id that is not loaded
 * returns 0. */
int64_t ffmi_rm_register_request_ex(ffmi_rm *rm, const int *prompt, int n_prompt,
                                    int max_length, int max_new_tokens,
                                    int add_special_tokens, int lora_id);
/* Run the serve loop until every registered request completes
 * (serve_incr_decoding / serve_spec_infer, request_manager.cc:3012-3173). */
ffmi_status ffmi_rm_serve_incr_decoding(ffmi_rm *rm, ffmi_model *llm);
ffmi_status ffmi_rm_serve_spec_infer(ffmi_rm *rm, ffmi_model *llm);
/* GenerationResult.output_tokens; returns count (or needed size) */
int ffmi_rm_get_output(ffmi_rm *rm, int64_t guid, int *tokens, int cap);
/* The log-probability of every output token given the tokens before it, when
 * the request was served by an LLM with ffmi_model_set_logprobs on: as many
 * entries as output tokens, prompt included (a prompt token's value is the
 * model's for that token, a generated token's the value of its pick); entry 0,
 * which has no predecessor, is 0.0.  Returns the count (or needed size), 0
 * when nothing was recorded, -1 for an unknown guid. */
int ffmi_rm_get_logprobs(ffmi_rm *rm, int64_t guid, float *out, int cap);
typedef struct {
  int llm_decoding_steps, ssm_decoding_steps;
  double start_us, finish_us, registration_us, first_token_us;
  int input_len, output_len;
} ffmi_profile;
ffmi_status ffmi_rm_get_profile(ffmi_rm *rm, int64_t guid, ffmi_profile *p);
/* aggregate counters of the last serve call */
typedef struct {
  long llm_steps, ssm_steps, tokens_committed, tree_tokens_verified;
  long request_verifies; /* (request, verify step) pairs that committed tokens */
  double wall_us;
  double llm_us, ssm_us; /* wall time inside LLM / SSM steps; the rest is host scheduling */
  long ssm_phases_chained; /* speculation phases run as chained beam steps (FFMI_SSM_CHAIN) */
  double ssm_exchange_us;  /* distributed SSMs: result exchange + remote bookkeeping */
} ffmi_serve_stats;
ffmi_status ffmi_rm_get_stats(ffmi_rm *rm, ffmi_serve_stats *s);



/* Test hooks: the residual RMSNorm folded into the decode GEMMs (T <= 32,
 * the path of LLaMA-7B decode steps; residual_rms_norm_kernels.cu:98-131
 * split over the GEMMs around it).  Producer: residual[T][out] += round(X .
 * W^T) in place (fp16 add) and ss_out[T][out/16] = per 16-column tile sums of
 * squares of the new residual.  Consumer: Y = (rmsnorm(residual) from ss_in
 * [T][in/16], weight norm_w, eps) . W^T, with the epilogue (FFMI_EPI_NONE /
 * FFMI_EPI_SILU_MUL, row-major).  Row-major fp16, no split-K. */
ffmi_status ffmi_debug_fused_residual_linear(const void *X, const void *W_packed, void *residual,
                                             float *ss_out, int T, int out_dim, int in_dim,
                                             ffmi_stream stream);
ffmi_status ffmi_debug_fused_norm_linear(const void *residual, const float *ss_in,
                                         const void *norm_w, float eps, const void *W_packed,
                                         void *Y, int T, int out_dim, int in_dim, int epilogue,
                                         ffmi_stream stream);

/* Test hooks: the consumers of deferred split-K slabs.  A split-K GEMM whose
 * consumer can combine leaves its partial sums as fp32 slabs [S][T][NP]
 * (NP >= the output width: the GEMM's padded tile columns); the value of
 * element (t, n) is fp16(slab 0 + slab 1 + ... in slab order), rounded once.
 * The public entry points never pass slabs (the in-library model does); each
 * hook below is one consumer fed with caller-made slabs: device memory,
 * 16-byte aligned, columns [width, NP) never read into a result.  Every
 * argument check is decided before any HIP call.
 *
 * ffmi_debug_partials_reduce: the reduce pass, Y[T][N] fp16 row-major.
 *   FFMI_ERR_INVALID: a null pointer, T < 0, S < 1, S > 16, NP % 16, N > NP,
 *   N < 1.
 * ffmi_debug_rmsnorm_partials: ffmi_rmsnorm_ex(x1, x2, ...) with x2 = the
 *   slabs' value (residual_out may alias x1, as the model calls it).
 *   FFMI_ERR_INVALID: a null x1 / slabs / w / out, no residual_out, T < 0,
 *   S < 1, S > 16, S > 8 with H > 1024, H > 8192, H < 8, H % 8, NP < H,
 *   NP % 4, unknown flags; FFMI_ERR_UNSUPPORTED: FFMI_Y_PACKED with H % 32.
 * ffmi_debug_attn_partials: ffmi_attn_inc / _spec / _tree (the handle's mode)
 *   with qkv [T][3 * heads * head_dim] = the slabs' value.
 *   FFMI_ERR_INVALID: a null pointer, a full-precision handle, S < 1, S > 8,
 *   NP < 3 * heads * head_dim, NP % 4.
 * ffmi_debug_allreduce_partials: ffmi_allreduce of this rank's [rows][cols]
 *   fp16 partial = the slabs' value, over an attached xGMI transport (the
 *   reduce pass folded into the copy-in).  FFMI_ERR_INVALID: a null pointer,
 *   S < 1, rows or cols < 0, no attached transport; then the transport's own
 *   status (FFMI_ERR_UNSUPPORTED: S > 8, NP < cols, NP % 4, cols % 8;
 *   nothing is launched). */
ffmi_status ffmi_debug_partials_reduce(const float *slabs, int S, int NP, void *Y, int T, int N,
                                       ffmi_stream stream);
ffmi_status ffmi_debug_rmsnorm_partials(const void *x1, const float *slabs, int S, int NP,
                                        const void *w, void *residual_out, void *out, int T, int H,
                                        float eps, int flags, ffmi_stream stream);
ffmi_status ffmi_debug_attn_partials(ffmi_attn *h, const ffmi_batch_dev *b, const float *slabs,
                                     int S, int NP, void *out, ffmi_stream stream);
ffmi_status ffmi_debug_allreduce_partials(ffmi_comm *c, const float *slabs, int S, int NP,
                                          void *out, int rows, int cols, ffmi_stream stream);
/* Test hook: the embedding lookup folded into layer 0's norm.  Over batch b's
 * tokens: residual_out[t] = table[id_t] (H halves per row) and out =
 * RMSNorm(residual_out) * w (flags: FFMI_Y_PACKED), where id_t is the token id,
 * or prev_ids[i] for a token id -1 - i (a chained beam step: entry i of the
 * previous step's top-k; prev_ids is device int32 and may be NULL when no id
 * is negative).  desc == NULL: b as last uploaded, its device blob read.
 * desc != NULL: desc is staged in b's pinned staging and NOT copied -- the
 * norm reads the staging and its grid copies the blob into b's device memory
 * for the step's later kernels (the model's fetch, in place of the H2D copy).
 * The ids must index the table / prev_ids: the caller's duty (the one id
 * check below is best effort: with desc == NULL it reads the blob last staged
 * on b, which is b's device blob only if ffmi_batch_upload or this hook
 * staged it).
 * FFMI_ERR_INVALID: a null b / table / w / residual_out / out, H < 8, H % 8,
 * H > 32768, unknown flags, a negative token id with prev_ids == NULL, what
 * ffmi_batch_upload refuses of desc; FFMI_ERR_UNSUPPORTED: FFMI_Y_PACKED with
 * H % 32. */
ffmi_status ffmi_debug_rmsnorm_gather(ffmi_batch_dev *b, const ffmi_batch_desc *desc,
                                      const void *table, const void *w, void *residual_out,
                                      void *out, int H, float eps, int flags,
                                      const int32_t *prev_ids, ffmi_stream stream);
/* Test hook: the output projection folded into the fused attention (small
 * models: head_dim 64, N <= 1024 output columns).  Runs ffmi_attn_inc / _spec
 * / _tree (the handle's mode) on batch b with qkv [T][3 * heads * 64] fp16 --
 * or, qkv == NULL, with the step's qkv as slabs [S][T][NP] under the rules of
 * ffmi_debug_attn_partials; exactly one of the two is given -- and asks the
 * launch to multiply each head's rounded fp16 output rows by that head's 64
 * columns of Wo_packed = ffmi_linear_pack_weight(Wo, N, heads * 64):
 *   slab[h][t][n] = sum_k out[t][h * 64 + k] * Wo[n][h * 64 + k]   (fp32)
 * for the T tokens of b, slab = [heads][T][N] with row stride T, not max_T
 * (max_T: the rows the caller's buffer holds per head).  The projection sums
 * slab over h in order and rounds once (ffmi_debug_rmsnorm_partials with
 * S = heads, NP = N).  *projected = 1.
 * An ineligible launch geometry is not an error: where the step is not one
 * work item per request, does not fit the fused kernel's LDS tail, has an
 * item of more than 16 queries or more than max_T tokens, or with
 * FFMI_ATTN_NO_FUSE set, the attention runs as usual, *projected = 0 and slab
 * is not touched (the caller runs the GEMM).  Every argument check is decided
 * before any HIP call.
 * FFMI_ERR_INVALID: a null h / b / out / Wo_packed / slab / projected, both
 * or neither of qkv and qkv_slabs, a full-precision handle, head_dim != 64,
 * N < 16, N % 16, N > 1024, max_T < 1, a slab not 16-byte aligned; with
 * qkv_slabs: not 16-byte aligned, S < 1, S > 8, NP < 3 * heads * 64, NP % 4. */
ffmi_status ffmi_debug_attn_oproj(ffmi_attn *h, const ffmi_batch_dev *b, const void *qkv,
                                  const float *qkv_slabs, int S, int NP, void *out,
                                  const void *Wo_packed, int N, float *slab, int max_T,
                                  int *projected, ffmi_stream stream);

/* Diagnostics: with FFMI_GEMM_STAMP set in the environment, M-split GEMM
 * launches record per-wave timestamps; copies the last launch's records
 * ({start, prologue done, k-loop done, end} at 100 MHz, HW_ID, XCC_ID) and
 * returns the number of waves (<= max_waves). */
long ffmi_debug_gemm_stamps(long long *dst, long max_waves);
/* Test hook: the launch ffmi_linear makes for these arguments (epilogue with
 * its layout flags), as plan = {path, MTW, NTW, S, mblocks, nblk}: path 0
 * skinny, 1 wave, 2 M-split, 3 the 256 x 256 tile form; row tiles per wave,
 * weight tiles per workgroup, split-K slices, row blocks and tile blocks of an
 * M-split launch (0, 0, 1, 0, 0 on the other paths).  FFMI_GEMM_PLAN is
 * honoured; the A/B-only forced skinny / wave forms are not reported.
 * Launches nothing and needs no device. */
ffmi_status ffmi_debug_gemm_plan(int T, int out_dim, int in_dim, int epilogue, int *plan /* [6] */);
/* Diagnostics: per-wave timeline of the last verify-size attention launch when
 * FFMI_ATTN_STAMP=1 (12 int64 per wave: start, after prologue, before the key
 * loop, after it, after the merge barrier, end, then [one-launch path] after
 * the commits, after the KV update, after its barrier, after the V^T stores
 * [100 MHz]; HW_ID, chunks). */
long ffmi_debug_attn_stamps(long long *dst, long max_waves);
/* FFMI_MARKERS=1 diagnostics: realtime-clock markers (100 MHz) enqueued
 * between the kernels of the model's last layer; copies up to n (<= 64). */
long ffmi_debug_markers(long long *dst, long n);

const char *ffmi_status_str(ffmi_status s);
/* message + file:line of the last failing check on this process */
const char *ffmi_last_error(void);
/* "ffmi 0.4 (gfx950)": 0.2 appended full_precision to ffmi_attn_cfg and
 * ffmi_model_opts (struct sizes changed) and added the *_f32 entry points;
 * 0.3 appended spec_extensions to ffmi_rm_config; 0.4 added top-p sampling
 * (ffmi_sample_topp, ffmi_sampling_counter, ffmi_model_set_sampling) and,
 * later under the same string (nothing that existed changed), its vocab-
 * sharded form: ffmi_vocab_shard_sample_scratch_bytes and
 * ffmi_vocab_shard_sample_topp; and the test hooks of the split-K slab
 * consumers and the gather norm: ffmi_debug_partials_reduce,
 * ffmi_debug_rmsnorm_partials, ffmi_debug_attn_partials,
 * ffmi_debug_allreduce_partials, ffmi_debug_rmsnorm_gather; and of the
 * output projection folded into the fused attention: ffmi_debug_attn_oproj;
 * and per-token log-probabilities: ffmi_token_logprobs(_workspace_bytes),
 * ffmi_model_set_logprobs, ffmi_rm_get_logprobs; and LoRA adapters on
 * down_proj: FFMI_MODEL_LORA, ffmi_model_lora_load(_folder) / _unload,
 * ffmi_lora_apply(_workspace_bytes), ffmi_rm_register_request_ex; and on the
 * attention projections: ffmi_model_lora_load_modules, _load_folder_ex,
 * ffmi_lora_apply_qkv, ffmi_lora_qkv_workspace_bytes */
const char *ffmi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FFMI_H_ */
