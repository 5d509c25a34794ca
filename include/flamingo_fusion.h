/*
 * libflamingo_fusion — C ABI of the MI355X (gfx950) Flamingo fusion path.
 *
 * This is the drop-in boundary below the Python modules: every entry point takes plain device pointers,
 * sizes and a HIP stream; no torch / C++ types; kernels are enqueued on the caller's stream and never
 * synchronise or allocate.  All tensors are caller-owned, 16-byte aligned, innermost dimension contiguous.
 * Return value: FF_OK or a negative error code; ff_last_error() gives a thread-local message.
 * State: none that is shared.  The entry points may be used from several threads on distinct streams / buffers; no environment variable is
 * read (the A/B switches of development builds exist only under -DFF_DEBUG, build.py --debug); every plan override travels in a
 * descriptor (ff_gemm_desc.split_k / tile / stages).  ff_last_error() is per thread, like errno.  The one process-wide object is the
 * opt-in launch-timing log of ff_gemm_profile_* (off by default): it has to see the launches of every thread - PyTorch issues backward
 * from its autograd worker thread - so recording into it is thread-safe (atomic slot counter), while enable / read / disable belong to
 * one controlling thread with no launch in flight.
 *
 * What each entry point replaces in the reference (dhansmair/flamingo-mini, paths relative to its root):
 *   ff_resampler_fwd/bwd     PerceiverResampler.forward + its autograd   flamingo_mini/perceiver_resampler.py:143-188
 *                            (PerceiverAttentionLayer.forward :32-96, FeedForward flamingo_mini/utils.py:22-50)
 *   ff_xattn_block_fwd/bwd   GatedCrossAttentionBlock.forward + autograd  flamingo_mini/gated_cross_attention.py:160-184
 *                            (MaskedCrossAttention.forward :42-131, cached K/V path :88-92,102-104)
 *   ff_text_time             media_locations.cumsum(dim=-1)               flamingo_mini/gated_cross_attention.py:97
 *   ff_quick_gelu_fwd/bwd    CLIP MLP activation (QuickGELU)               transformers CLIPMLP via modeling_flamingo.py:70-78
 *   ff_shifted_ce_fwd/bwd    shifted F.cross_entropy on the logits        flamingo_mini/modeling_flamingo.py:288-298
 *   ff_shifted_ce_fwd/bwd_reg  the same with label smoothing and z-loss   HF Trainer --label_smoothing_factor (trainer_pt_utils.LabelSmoother)
 *   ff_adamw_step            torch AdamW over parameters_trainable()      training/train.sh:10-13, modeling_flamingo.py:132-138
 * The primitive entry points (ff_gemm, ff_layernorm_*, ff_attention_*, ff_rows_reduce, ff_gate_grad) are the
 * kernels those are built from; they are exported so each can be parity-tested on its own.
 */
#ifndef FLAMINGO_FUSION_H
#define FLAMINGO_FUSION_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the declarations of this header are exported (tests/test_cabi.py compares the
 * dynamic symbol table of the built .so with them). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct ihipStream_t* ff_stream_t; /* == hipStream_t */

enum { FF_OK = 0, FF_ERR_SHAPE = -1, FF_ERR_UNSUPPORTED = -2, FF_ERR_WORKSPACE = -3, FF_ERR_LAUNCH = -4 };
enum { FF_DTYPE_F32 = 0, FF_DTYPE_BF16 = 1 };
enum { FF_ACT_NONE = -1, FF_ACT_GELU = 0, FF_ACT_SQRELU = 1, FF_ACT_RELU = 2 }; /* utils.py:26-30 */

int ff_version(void);          /* ABI version, bumped on any signature change (3: ff_gemm_desc.tile / .stages replace ff_gemm_set_tuning;
                                * 4: ff_xattn_desc.sync, ff_xattn_sync_bytes / _status, ff_resampler_layer_* / _prologue_* / _epilogue_*;
                                * 5: gradient clipping: ff_grad_sumsq*, ff_grad_clip_coef, ff_scale_grads, ff_adamw_step_clipped;
                                * 6: fp32 gradient accumulation: ff_grad_accumulate, ff_adamw_step_acc;
                                * still 6, additions only: the non-finite gradient guard ff_grad_guard, ff_adamw_step_guarded;
                                * still 6, addition only: token selection for sampled decoding, ff_sample_token;
                                * still 6, additions only: beam search on the captured decode step, ff_beam_step, ff_beam_gather;
                                * still 6, additions only: stochastic rounding for pure-bf16 training, ff_adamw_step_sr, ff_stochastic_round_bf16;
                                * still 6, addition only: logits processors on the captured decode step, ff_logits_process;
                                * still 6, addition only: exponential moving average of the weights, ff_ema_update;
                                * still 6, addition only: log-probability of the chosen token on the captured decode step, ff_token_logprob;
                                * still 6, addition only: constrained decoding on the captured decode step (candidate trie, bad words), ff_logits_constrain;
                                * still 6, addition only: diverse beam search on the captured decode step, ff_group_beam_step;
                                * still 6, addition only: classifier-free guidance on the captured decode step, ff_guided_logits;
                                * still 6, addition only: truncation samplers (min_p, typical_p, epsilon / eta cutoff), ff_sample_token_truncated;
                                * still 6, addition only: exact closed-set scoring over a candidate trie, ff_logprob_gather;
                                * still 6, additions only: beam sampling on the captured decode step, ff_beam_sample_step, ff_beam_sample_noise;
                                * still 6, additions only: contrastive search on the captured decode step, ff_topk_logprob, ff_contrastive_step) */
const char* ff_arch(void);     /* "gfx950" */
const char* ff_last_error(void);

/* Row addressing shared by the row-wise kernels and the GEMM operands:
 * logical row r lives at  base + (r / rows_per_seg) * seg_stride + (r % rows_per_seg) * ld   (elements).
 * rows_per_seg <= 0: plain row-major with leading dimension ld.  seg_stride == 0 broadcasts one segment. */
typedef struct ff_rowmap {
    long long ld;
    long long seg_stride;
    int rows_per_seg;
    int reserved;
} ff_rowmap;

/* ------------------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:   v = scale * sum_k A[m,k] * B[k,n]
 *                             aux_out[m,n] = v                      (if aux_out)
 *                             v *= tanh(*gate)                      (if gate: device scalar of `dtype`)
 *                             v  = act(v)                           (if act >= 0)
 *                             v *= act'(aux_in[m,n])                (if act_bwd >= 0)
 *                             C[m,n] = v + residual[m,n]            (residual optional)
 * a_layout 0: A stored [M][K] (nn.Linear input);  1: A stored [K][M] (used for weight gradients, A = dY^T)
 * b_layout 0: B stored [N][K] (nn.Linear weight (out,in));  1: B stored [K][N]
 * a_map/b_map address the STORED rows (M or K rows of A; N or K rows of B); c_map addresses C, aux_*, residual.
 * split_k > 1 needs workspace of ff_gemm_workspace_bytes().
 * ------------------------------------------------------------------------------------------------------ */
typedef struct ff_gemm_desc {
    int dtype;
    int M, N, K;
    int a_layout, b_layout;
    ff_rowmap a_map, b_map, c_map;
    float scale;
    int act;      /* FF_ACT_* or FF_ACT_NONE */
    int act_bwd;  /* FF_ACT_* or FF_ACT_NONE */
    int split_k;  /* 0 = choose automatically */
    int tile;     /* bf16 block tile: 0 = choose automatically; 128 = 128x128 (4 waves), 6412 = 64x128, 64 = 64x64,
                   * 64002 / 128002 = 64x64 / 128x128 producer/consumer (8 waves), 128160 = 128x160 producer/consumer (A K-major only),
                   * 128168 = the same 128x160 tile with eight MFMA waves (4 x 2) + four DMA waves,
                   * 256128 = 256x128 producer/consumer, eight MFMA + eight DMA waves (chosen automatically for products with >= 4096 rows and a K-major A; with an
                   *          M-major A - weight gradients - eight MFMA + four DMA waves, selectable only),
                   * 256256 = 256x256 on sixteen waves that both issue the DMA and run the MFMAs (both operands K-major; `stages` ignored; chosen
                   *          automatically for such products with >= 4096 rows, >= 2048 contraction elements and at least one tile per CU),
                   * 3264 = 32x64 producer/consumer (decode: M <= 32 rows; both operands K-major),
                   * 3216 = weight-streaming kernel for M <= 32 rows (16 output columns per workgroup, no LDS staging; K-major operands, K % 32 == 0) */
    int stages;   /* depth of the LDS operand ring: 0 = default, 2..4 */
} ff_gemm_desc;

size_t ff_gemm_workspace_bytes(const ff_gemm_desc* d);
int ff_gemm(const ff_gemm_desc* d, const void* A, const void* B, void* C, void* aux_out, const void* aux_in,
            const void* residual, const void* gate, void* workspace, size_t workspace_bytes, ff_stream_t stream);


/* Optional measurement aid (bench.py's roofline leg): while enabled, every GEMM main-kernel launch is bracketed by two
 * HIP events on its own stream.  ff_gemm_profile_read() waits for the recorded launches, fills `out` (returns the count)
 * and clears the log.  ff_gemm_profile_enable(0) switches it off.  Recording is thread-safe (launches of any thread on any stream claim
 * their slot atomically); enable / read / disable belong to ONE controlling thread, called while no launch is in flight.
 * `tile` < 0 marks the non-GEMM launches: -1 / -2 / -3 attention core (forward, dQ, dK / dV); -4 / -6 / -8 the fused cross-attention
 * forward (b_layout = the resident kernel's ring depth, 0 = the general kernel) and -5 / -7 / -9 its backward; -10 / -11 the decode
 * feed-forward for <= 32 rows (LayerNorm + up-projection; down-projection + gate + residual, split_k = K slices combined in the launch). */
typedef struct ff_gemm_profile_record {
    int dtype, tile, a_layout, b_layout;
    int M, N, K, nz, split_k;
    float ms;
} ff_gemm_profile_record;
int ff_gemm_profile_enable(int max_records);
int ff_gemm_profile_read(ff_gemm_profile_record* out, int max_records);
/* Introspection: block tile and split-K factor ff_gemm would choose for this problem (no device access). */
int ff_gemm_plan(const ff_gemm_desc* d, int* bm, int* bn, int* split_k);

/* ------------------------------------------------------------------------------------------------------
 * LayerNorm over the last axis (eps inside the sqrt, biased variance: torch.nn.LayerNorm).
 * Optional broadcast addend fused in front: x[r] += add[((r % add_rows_per_seg) / add_div)]  — the
 * time_pos_emb add of perceiver_resampler.py:166.
 * fwd: stats_given != 0 reuses mean/rstd instead of recomputing; y == NULL computes the statistics only.
 * bwd: dx = dx_residual + LN'(dy) (dx_residual optional, may alias dx); dgamma/dbeta are written, not accumulated.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct ff_ln_desc {
    int dtype;
    int rows, cols;
    ff_rowmap x_map;  /* x (fwd, bwd) */
    ff_rowmap y_map;  /* y (fwd) / dy (bwd) */
    ff_rowmap dx_map; /* dx and dx_residual (bwd) */
    int add_rows_per_seg, add_div;
    float eps;
    int stats_given;
} ff_ln_desc;

int ff_layernorm_fwd(const ff_ln_desc* d, const void* x, const void* add, const void* gamma, const void* beta,
                     void* y, float* mean, float* rstd, ff_stream_t stream);
size_t ff_layernorm_bwd_workspace_bytes(const ff_ln_desc* d);
int ff_layernorm_bwd(const ff_ln_desc* d, const void* dy, const void* x, const void* add, const void* gamma,
                     const float* mean, const float* rstd, void* dx, const void* dx_residual, void* dgamma,
                     void* dbeta, void* workspace, size_t workspace_bytes, ff_stream_t stream);

/* out[g][c] = sum over rows r with group(r) == g of x[r][c],  group(r) = (r % rows_per_batch) / rows_per_group.
 * (d latents: rows_per_batch = q, rows_per_group = 1;  d time_pos_emb: rows_per_batch = T*v, rows_per_group = v) */
typedef struct ff_reduce_desc {
    int dtype;
    int rows, cols;
    ff_rowmap x_map;
    int rows_per_batch, rows_per_group;
} ff_reduce_desc;
size_t ff_rows_reduce_workspace_bytes(const ff_reduce_desc* d);
int ff_rows_reduce(const ff_reduce_desc* d, const void* x, void* out, void* workspace, size_t workspace_bytes,
                   ff_stream_t stream);

/* d alpha = (1 - tanh(alpha)^2) * sum(a .* b) over rows x cols  (gated_cross_attention.py:180,182 backward) */
size_t ff_gate_grad_workspace_bytes(int rows, int cols);
int ff_gate_grad(int dtype, int rows, int cols, const void* a, const void* b, const void* alpha, void* dalpha,
                 void* workspace, size_t workspace_bytes, ff_stream_t stream);

/* text_time[b][i] = sum_{j<=i} media_locations[b][j]   (media_locations: int64 / int32 / uint8(bool)) */
int ff_text_time(int batch, int n_tokens, const void* media_locations, int elem_bytes, int* text_time,
                 ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Attention core  O = softmax(Q K^T) V  over row ranges, never materialising the score matrix.
 *   mode FF_ATTN_DENSE : every query attends to all n_kv keys (resampler, perceiver_resampler.py:85-92)
 *   mode FF_ATTN_MEDIA : query i attends to the n_visual keys of image text_time[b][i]
 *                        (gated_cross_attention.py:97-123): text_time == 0 -> output row 0 and no gradient;
 *                        text_time > n_kv / n_visual -> uniform average over all keys (fully masked row).
 * Q is expected pre-scaled.  Element (b, row, h, d) of a tensor lives at base + b*sb + row*sr + h*sh + d.
 * lse[b][h][row] (fp32) is saved by fwd and consumed by bwd.
 * ------------------------------------------------------------------------------------------------------ */
enum { FF_ATTN_DENSE = 0, FF_ATTN_MEDIA = 1 };
typedef struct ff_strides {
    long long sb, sr, sh;
} ff_strides;
typedef struct ff_attn_desc {
    int dtype;
    int batch, heads, dim_head;
    int n_q, n_kv;
    int mode, n_visual;
    int tt_stride;   /* row stride of text_time (elements); query i of batch b reads text_time[b*tt_stride + tt_offset + i] */
    int tt_offset;
    ff_strides q, k, v, o;      /* forward tensors; dq/dk/dv/do use dq, dk, dv, dout strides below */
    ff_strides dq, dk, dv, dout;
} ff_attn_desc;

int ff_attention_fwd(const ff_attn_desc* d, const void* Q, const void* K, const void* V, const int* text_time,
                     void* O, float* lse, ff_stream_t stream);
size_t ff_attention_bwd_workspace_bytes(const ff_attn_desc* d);
int ff_attention_bwd(const ff_attn_desc* d, const void* Q, const void* K, const void* V, const int* text_time,
                     const void* O, const void* dO, const float* lse, void* dQ, void* dK, void* dV,
                     void* workspace, size_t workspace_bytes, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * PerceiverResampler (perceiver_resampler.py:99-188).
 * x_f: (batch, n_frames, n_tokens, dim) contiguous; out: (batch, num_latents, dim).
 * params / grads: arrays of device pointers in this order (names = reference state_dict keys):
 *   [0] latents  [1] time_pos_emb  [2] norm.weight  [3] norm.bias
 *   then per layer i, base = 4 + 12*i:
 *   +0 layers.i.0.norm_media.weight  +1 .norm_media.bias  +2 .norm_latents.weight  +3 .norm_latents.bias
 *   +4 layers.i.0.to_q.weight  +5 .to_k.weight  +6 .to_v.weight  +7 .to_out.weight
 *   +8 layers.i.1.0.weight  +9 layers.i.1.0.bias  +10 layers.i.1.1.weight  +11 layers.i.1.3.weight
 * `saved` persists fwd -> bwd (activations, statistics); `scratch` is transient.
 * bwd writes every gradient (no accumulation); dx_f may be NULL (CLIP frozen) — d time_pos_emb is still exact.
 * This is the whole stack in one call, like the reference's own call site (modeling_flamingo.py:176 calls the module once): only the
 * stack-level call can group the weight gradients of four layers per launch and finish all 3 * depth + 1 LayerNorm-backward reductions
 * with three launches.  SURVEY.md 8-b2's per-layer export set (ff_resampler_layer_fwd/bwd + prologue / epilogue) follows below; it is what
 * a data-parallel caller uses (one gradient bucket per layer).
 * ------------------------------------------------------------------------------------------------------ */
#define FF_RESAMPLER_GLOBAL_PARAMS 4
#define FF_RESAMPLER_LAYER_PARAMS 12
typedef struct ff_resampler_desc {
    int dtype;
    int batch, n_frames, n_tokens, dim;
    int depth, heads, dim_head, num_latents, num_time_embeds, ff_mult, act;
} ff_resampler_desc;
size_t ff_resampler_saved_bytes(const ff_resampler_desc* d);
size_t ff_resampler_scratch_bytes(const ff_resampler_desc* d);
int ff_resampler_fwd(const ff_resampler_desc* d, const void* x_f, const void* const* params, void* out,
                     void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, ff_stream_t stream);
int ff_resampler_bwd(const ff_resampler_desc* d, const void* x_f, const void* const* params, const void* dout,
                     const void* saved, size_t saved_bytes, void* const* grads, void* dx_f, void* scratch,
                     size_t scratch_bytes, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * PerceiverResampler, ONE LAYER PER CALL (ABI 4; SURVEY.md 8-b2's minimum export set; perceiver_resampler.py:181-183 is a per-layer loop).
 *   forward :  prologue_fwd (statistics of x_f + time_pos_emb, :166 / :52, shared by every layer's norm_media)
 *              -> depth x layer_fwd (x = x + attn(x_f, x); x = x + ffw(x), :182-183; layer 0 takes the latents (num_latents, dim) with
 *                 x_in_is_latents = 1: they are broadcast over the batch, :179)
 *              -> epilogue_fwd (final LayerNorm, :187)
 *   backward:  epilogue_bwd -> depth x layer_bwd (last layer first) -> prologue_bwd
 * layer_params / layer_grads: the 12 pointers of ONE layer in the order of ff_resampler_fwd's per-layer block (+0 norm_media.weight ... +11
 * layers.i.1.3.weight).  layer_bwd writes every one of the layer's parameter gradients - final when the call returns: a data-parallel
 * caller gets one gradient bucket per layer, which can leave while the layer below runs backward - and d x_in (batch, num_latents, dim) (for
 * layer 0: the gradient of the BROADCAST latents; prologue_bwd sums it over the batch), and adds its share of d x_f to `dx_f`
 * (dx_f_accumulate = 0 for the first layer_bwd call of a pass, which overwrites).  prologue_bwd: d latents, d time_pos_emb (complete).
 * ff_resampler_desc.depth is ignored by these calls.  `saved` buffers persist fwd -> bwd; every `scratch` is ff_resampler_layer_scratch_bytes().
 * The stack-level ff_resampler_fwd / _bwd above remain the single-GPU fast path (they group the weight gradients of four layers per
 * launch and finish all LayerNorm-backward reductions with three launches).
 * ------------------------------------------------------------------------------------------------------ */
size_t ff_resampler_prologue_saved_bytes(const ff_resampler_desc* d);
size_t ff_resampler_layer_saved_bytes(const ff_resampler_desc* d);
size_t ff_resampler_layer_scratch_bytes(const ff_resampler_desc* d);
size_t ff_resampler_epilogue_saved_bytes(const ff_resampler_desc* d);
int ff_resampler_prologue_fwd(const ff_resampler_desc* d, const void* x_f, const void* time_pos_emb, void* saved_pro, size_t saved_pro_bytes,
                              ff_stream_t stream);
int ff_resampler_layer_fwd(const ff_resampler_desc* d, const void* x_f, const void* time_pos_emb, const void* saved_pro, size_t saved_pro_bytes,
                           const void* x_in, int x_in_is_latents, const void* const* layer_params, void* x_out, void* saved, size_t saved_bytes,
                           void* scratch, size_t scratch_bytes, ff_stream_t stream);
int ff_resampler_epilogue_fwd(const ff_resampler_desc* d, const void* x_last, const void* norm_weight, const void* norm_bias, void* out,
                              void* saved_epi, size_t saved_epi_bytes, ff_stream_t stream);
int ff_resampler_epilogue_bwd(const ff_resampler_desc* d, const void* dout, const void* x_last, const void* norm_weight, const void* saved_epi,
                              size_t saved_epi_bytes, void* dx_last, void* d_norm_weight, void* d_norm_bias, void* scratch, size_t scratch_bytes,
                              ff_stream_t stream);
int ff_resampler_layer_bwd(const ff_resampler_desc* d, const void* x_f, const void* time_pos_emb, const void* saved_pro, size_t saved_pro_bytes,
                           const void* x_in, int x_in_is_latents, const void* const* layer_params, const void* dx_out, const void* saved,
                           size_t saved_bytes, void* const* layer_grads, void* dx_in, void* dx_f, int dx_f_accumulate, void* scratch,
                           size_t scratch_bytes, ff_stream_t stream);
int ff_resampler_prologue_bwd(const ff_resampler_desc* d, const void* dx0, const void* dx_f, void* d_latents, void* d_time_pos_emb, void* scratch,
                              size_t scratch_bytes, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * GatedCrossAttentionBlock (gated_cross_attention.py:135-184).
 * y: (batch, n_tokens, dim); visual_features: (batch, n_media, n_visual, dim_visual); text_time from ff_text_time.
 * params / grads order:
 *   [0] alpha_attn [1] alpha_ffw [2] attn.norm.weight [3] attn.norm.bias [4] attn.to_q.weight
 *   [5] attn.to_kv.weight [6] attn.to_out.weight [7] ffw.0.weight [8] ffw.0.bias [9] ffw.1.weight [10] ffw.3.weight
 * Cached decode (previous_kv): pass cached_k/cached_v (+ strides) and visual_features = NULL; n_media is then
 * n_kv / n_visual and text_time rows are read at tt_offset (the last n_tokens entries, :102-104).
 * Uncached: K/V are produced in `saved` at ff_xattn_kv_offset() as (batch, n_media*n_visual, 2, heads, dim_head).
 * Non-zero cached_k / cached_v strides in the descriptor <=> K / V come from outside (cached decode or ff_kv_project_fwd); `saved`
 * then holds no K/V region (size queries and calls must use the same descriptor).
 * `sync` (ABI 4, optional): ff_xattn_sync_bytes() bytes of device memory that were ZERO when first handed to the library and that only the
 * library writes afterwards.  With it, and at the training / decode shape of the published configurations (bf16, 8 heads of 64, at most 32
 * tokens and 64 keys per sample, dim a multiple of 256 up to 1280 - at 1536 the backward kernel's resident rows + ring + tiles are 165 184 B
 * of LDS, over the CU's 160 KiB, and the block keeps its separate launches -, batch <= FF_XATTN_SYNC_SLOTS, and a device that reports 8 XCDs
 * of at least 16 CUs each: see "Co-residency" in csrc/ff_xattn_fused.hip), `to_out` + tanh gate + residual
 * (gated_cross_attention.py:124-126,180) run INSIDE the fused LayerNorm -> to_q -> attention launch, and d LN(y) = d q . Wq inside the fused
 * attention-backward launch: the eight (sample, head) workgroups of a sample exchange their tiles through per-sample arrival counters in
 * `sync` instead of through a kernel boundary (two 64 x 64-tile GEMM launches per block and step less).  At the training shape the
 * LayerNorm behind each of those outputs runs in the same launch as well - forward: LN(y1) of the feed-forward (utils.py:46); backward: the
 * LayerNorm backward of LN(y) - with the rows' statistics making one more trip through a second bank of counters (two more launches per block
 * and step less).  Calls that share a `sync` buffer must be ordered on one stream (the counters are per sample, not per call); NULL keeps the
 * separate launches.  Results are the same either way up to the rounding of fp32 sums taken in another order; the word behind the first two
 * banks is an error flag (ff_xattn_sync_status; non-zero: an arrival wait timed out - a launch was denied co-residency of a sample's eight
 * workgroups - and that call's output is invalid).  A caller MUST read that flag before trusting results computed with a `sync` buffer: the
 * Python layer does so after warm-up steps, every N graph replays, at every eager optimizer step (non-blocking) and at the end of bench.py.
 * ------------------------------------------------------------------------------------------------------ */
#define FF_XATTN_PARAMS 11
#define FF_XATTN_SYNC_SLOTS 1024
typedef struct ff_xattn_desc {
    int dtype;
    int batch, n_tokens, dim, dim_visual;
    int n_media, n_visual, heads, dim_head, ff_mult, act;
    int tt_stride, tt_offset;
    ff_strides cached_k, cached_v; /* used only when cached_k != NULL */
    void* sync;                    /* see above; NULL = none */
} ff_xattn_desc;
size_t ff_xattn_sync_bytes(void);              /* (4 * FF_XATTN_SYNC_SLOTS + 64) * 4: two banks of per-sample counters each way + a status word */
int ff_xattn_sync_status(const void* sync, ff_stream_t stream);   /* synchronises `stream`; 0 = no wait ever timed out, 1 = one did, < 0 = error */
size_t ff_xattn_saved_bytes(const ff_xattn_desc* d);
size_t ff_xattn_scratch_bytes(const ff_xattn_desc* d);
size_t ff_xattn_kv_offset(const ff_xattn_desc* d);
/* Where ff_xattn_block_fwd leaves the LayerNorm by-products that the backward reads, inside `saved` (host only; for tests and tools).
 * mean_a / rstd_a: fp32 (batch * n_tokens) statistics of attn.norm; yn = attn.norm(y); y1 = y + tanh(alpha_attn) * to_out(...);
 * mean_f / rstd_f: statistics of ffw.0 over y1; xn_f = ffw.0(y1).  yn, y1 and xn_f are (batch * n_tokens, dim) in the descriptor's dtype.
 * The other stages' results, selectors 7..13 (additions; the numbering above is unchanged): Qs = scale * to_q(yn) and O, the attention's
 * output, (batch * n_tokens, heads * dim_head); lse, fp32 (batch, heads, n_tokens), 1e30 for a row that sees no key; attn_out = to_out(O),
 * (batch * n_tokens, dim); Hpre = ffw.1(xn_f) and Aact = act(Hpre), (batch * n_tokens, ff_mult * dim); ffw_out = ffw.3(Aact), (batch *
 * n_tokens, dim).  In memory the regions follow each other as mean_a, rstd_a, yn, Qs, lse, O, attn_out, y1, mean_f, rstd_f, xn_f, Hpre,
 * Aact, ffw_out.
 * Returns FF_OK and the region's byte offset and size, or FF_ERR_SHAPE for a bad descriptor, selector or pointer. */
enum { FF_XA_SAVED_MEAN_A = 0, FF_XA_SAVED_RSTD_A = 1, FF_XA_SAVED_YN = 2, FF_XA_SAVED_Y1 = 3, FF_XA_SAVED_MEAN_F = 4, FF_XA_SAVED_RSTD_F = 5,
       FF_XA_SAVED_XN_F = 6, FF_XA_SAVED_QS = 7, FF_XA_SAVED_LSE = 8, FF_XA_SAVED_O = 9, FF_XA_SAVED_ATTN_OUT = 10, FF_XA_SAVED_HPRE = 11,
       FF_XA_SAVED_AACT = 12, FF_XA_SAVED_FFW_OUT = 13 };
int ff_xattn_saved_view(const ff_xattn_desc* d, int what, size_t* offset, size_t* bytes);
int ff_xattn_block_fwd(const ff_xattn_desc* d, const void* y, const void* visual_features, const int* text_time,
                       const void* const* params, const void* cached_k, const void* cached_v, void* y_out,
                       void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, ff_stream_t stream);
int ff_xattn_block_bwd(const ff_xattn_desc* d, const void* y, const void* visual_features, const int* text_time,
                       const void* const* params, const void* dy_out, const void* saved, size_t saved_bytes,
                       void* const* grads, void* dy, void* dvisual_features, void* scratch, size_t scratch_bytes,
                       ff_stream_t stream);


/* ------------------------------------------------------------------------------------------------------
 * Key / value projection hoisted out of the cross-attention layers.  gated_cross_attention.py:84-86 applies every layer's
 * `to_kv` to the SAME visual features; projecting for all layers in grouped launches (and summing d visual_features once)
 * replaces n_layers small GEMMs per direction.  w_kv[l] (kv_dim, dim_visual) = layer l's to_kv.weight; kv_out[l] / dkv[l]
 * (rows, kv_dim) with rows = batch * n_media * n_visual, K = columns [0, kv_dim/2), V = the rest - the layout
 * ff_xattn_block_fwd expects for cached_k / cached_v with strides {n_kv * kv_dim, kv_dim, dim_head}.
 * Training step:  ff_kv_project_fwd -> per layer ff_xattn_block_fwd(cached_k = kv_out[l], cached_v = kv_out[l] + kv_dim/2)
 *                 ... per layer ff_xattn_block_bwd_kv(... dkv[l]) -> ff_kv_project_bwd (d to_kv.weight of every layer, d visual_features).
 * ------------------------------------------------------------------------------------------------------ */
typedef struct ff_kvproj_desc {
    int dtype;
    int n_layers;
    int rows;         /* batch * n_media * n_visual */
    int dim_visual;
    int kv_dim;       /* 2 * heads * dim_head */
} ff_kvproj_desc;
size_t ff_kv_project_workspace_bytes(const ff_kvproj_desc* d, int with_dvisual_features);
int ff_kv_project_fwd(const ff_kvproj_desc* d, const void* visual_features, const void* const* w_kv, void* const* kv_out,
                      void* workspace, size_t workspace_bytes, ff_stream_t stream);
int ff_kv_project_bwd(const ff_kvproj_desc* d, const void* visual_features, const void* const* w_kv, const void* const* dkv,
                      void* const* dw_kv, void* dvisual_features, void* workspace, size_t workspace_bytes, ff_stream_t stream);
/* Backward of a block whose K / V came from ff_kv_project_fwd (d->cached_k / cached_v = their strides): writes d K / d V into
 * `dkv` (same layout as kv_out[l]); grads[5] (to_kv.weight) is not written. */
int ff_xattn_block_bwd_kv(const ff_xattn_desc* d, const void* y, const void* k, const void* v, const int* text_time,
                          const void* const* params, const void* dy_out, const void* saved, size_t saved_bytes, void* const* grads,
                          void* dy, void* dkv, void* scratch, size_t scratch_bytes, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Deferred, grouped weight gradients.  The four weight-gradient GEMMs of a block (d ffw.3.weight, d ffw.1.weight,
 * d attn.to_out.weight, d attn.to_q.weight = 1/3 of its FLOPs) are not on the critical path of backward and a single one
 * fills a third of the chip.  ff_xattn_block_bwd_kv_data is ff_xattn_block_bwd_kv without them: it leaves their operands
 * (d y1, d H, d Qs) in the caller-owned `stash`; ff_xattn_wgrad_grouped then computes them for up to FF_WGRAD_GROUP_MAX
 * same-shaped blocks per call in four grouped launches.  grads[5] (to_kv) is never written.  The LayerNorm / gate gradients
 * (grads[0..3], [7], [8]) are COMPLETE only after the grouped call as well: the data pass runs the one-pass LayerNorm backward and
 * leaves its per-workgroup partial sums in the stash; the grouped call reduces those of all its blocks with one launch (72 -> 9
 * launches per step, none of them on the data-gradient chain, at flamingo-mini's size).  For that the data pass requires y, dy_out, dy and the two
 * LayerNorm weight vectors to be 16-byte aligned (FF_ERR_SHAPE otherwise; use ff_xattn_block_bwd_kv for odd views).
 * `params` / `grads` of the grouped call: n_blocks * FF_XATTN_PARAMS pointers, block after block, the SAME gradient pointers the
 * data pass received; dy_out / saved / stash: one pointer per block (the buffers of that block's data pass).
 * ------------------------------------------------------------------------------------------------------ */
#define FF_WGRAD_GROUP_MAX 12
size_t ff_xattn_wgrad_stash_bytes(const ff_xattn_desc* d);
/* Where ff_xattn_block_bwd_kv_data leaves the three operands inside `stash` (host only; for tests and tools, as ff_xattn_saved_view):
 * d y1 (batch * n_tokens, dim), d H (batch * n_tokens, ff_mult * dim), the gradient of Hpre, and d Qs (batch * n_tokens, heads * dim_head),
 * in this order and in the descriptor's dtype. */
enum { FF_XA_STASH_DY1 = 0, FF_XA_STASH_DH = 1, FF_XA_STASH_DQS = 2 };
int ff_xattn_wgrad_stash_view(const ff_xattn_desc* d, int what, size_t* offset, size_t* bytes);
size_t ff_xattn_wgrad_workspace_bytes(const ff_xattn_desc* d);
int ff_xattn_block_bwd_kv_data(const ff_xattn_desc* d, const void* y, const void* k, const void* v, const int* text_time,
                               const void* const* params, const void* dy_out, const void* saved, size_t saved_bytes, void* const* grads,
                               void* dy, void* dkv, void* stash, size_t stash_bytes, void* scratch, size_t scratch_bytes, ff_stream_t stream);
int ff_xattn_wgrad_grouped(const ff_xattn_desc* d, int n_blocks, const void* const* dy_out, const void* const* saved, size_t saved_bytes,
                           const void* const* stash, size_t stash_bytes, const void* const* params, void* const* grads, void* workspace,
                           size_t workspace_bytes, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Fused multi-tensor AdamW over the trainable parameters (the reference trains with `--optim adamw_torch`,
 * training/train.sh:10-13; parameters_trainable() modeling_flamingo.py:132-138).  All tensors of one call share `dtype`
 * (params, grads and both moment buffers); math is fp32.  step is the 1-based step count AFTER incrementing
 * (bias corrections 1 - beta^step).  grad_scale multiplies every gradient first (0 = 1.0; e.g. 1/world after a SUM all-reduce).
 * ------------------------------------------------------------------------------------------------------ */
typedef struct ff_adamw_desc {
    int dtype;
    int n_tensors;
    int step;
    float lr, beta1, beta2, eps, weight_decay, grad_scale;
    const float* step_dev;   /* optional device scalar holding the step count (>= 1): used instead of `step`, so the launch can be
                              * replayed from a captured HIP graph while the caller advances the counter on the device */
} ff_adamw_desc;
int ff_adamw_step(const ff_adamw_desc* d, void* const* params, const void* const* grads, void* const* exp_avg,
                  void* const* exp_avg_sq, const long long* numels, ff_stream_t stream);
/* Mixed-precision variant (the reference trains with `--fp16` autocast, i.e. fp32 master weights and fp32 Adam moments,
 * training/train.sh:24): parameters / gradients in d->dtype, the two moments in `state_dtype` (d->dtype or FF_DTYPE_F32), and -
 * for bf16 parameters - optional fp32 `master` copies: the update is applied to the master copy and the bf16 parameter is its
 * rounding, written by the same kernel.  `lr_dev` (optional device scalar) replaces d->lr, so a learning-rate schedule stays
 * effective when the launch is replayed from a captured HIP graph. */
int ff_adamw_step_mixed(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, void* const* exp_avg,
                        void* const* exp_avg_sq, float* const* master, const float* lr_dev, const long long* numels, ff_stream_t stream);
/* ff_adamw_step_mixed with every gradient multiplied by the device scalar *grad_coef as it is read (one fp32 factor grad_scale * *grad_coef):
 * gradient clipping by global norm (ABI 5) with the coefficient of ff_grad_clip_coef, without touching the gradients in memory. */
int ff_adamw_step_clipped(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, void* const* exp_avg,
                          void* const* exp_avg_sq, float* const* master, const float* lr_dev, const float* grad_coef, const long long* numels,
                          ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Gradient clipping by global L2 norm (ABI 5): torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2), which the reference's
 * HF Trainer applies before every optimizer step (TrainingArguments.max_grad_norm, default 1.0).  Everything stays on the device:
 *   ff_grad_sumsq          sum of squares of (scale * g) over n_tensors contiguous gradients of one dtype; ONE fp32 partial per
 *                          workgroup in partials[0 .. ff_grad_sumsq_partials(n_tensors, numels) - 1] (fixed slots, no atomics: the total
 *                          is reproducible bit for bit).  Offset `partials` to continue the slots of an earlier call (another dtype,
 *                          another bucket); n_partials is the room left there (FF_ERR_WORKSPACE if too small).
 *   ff_grad_sumsq_reduce   one workgroup: *sum = (accumulate ? *sum : 0) + the n_partials partials, added in fp64 in a fixed order.  A
 *                          data-parallel caller all-reduces *sum between this and the next call.
 *   ff_grad_clip_coef      *norm = sqrt(*sum) (fp32), *coef = min(1, max_norm / (*norm + 1e-6)); either output may be null.  A non-finite
 *                          norm propagates as in torch (NaN coefficient for a NaN norm, 0 for an infinite one).
 *   ff_scale_grads         g *= *coef in place over n_tensors contiguous gradients of one dtype (fp32 math).
 * ------------------------------------------------------------------------------------------------------ */
long long ff_grad_sumsq_partials(int n_tensors, const long long* numels);
int ff_grad_sumsq(int dtype, int n_tensors, const void* const* grads, const long long* numels, float scale, float* partials,
                  long long n_partials, ff_stream_t stream);
int ff_grad_sumsq_reduce(const float* partials, long long n_partials, double* sum, int accumulate, ff_stream_t stream);
int ff_grad_clip_coef(const double* sum, float max_norm, float* norm, float* coef, ff_stream_t stream);
int ff_scale_grads(int dtype, int n_tensors, void* const* grads, const long long* numels, const float* coef, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * fp32 gradient accumulation over micro-batches (ABI 6): HF Trainer's --gradient_accumulation_steps (training/train.sh) without the bf16
 * `grad += g` of autograd, which rounds the running sum to 8 significant bits after every micro-batch.
 *   ff_grad_accumulate     acc[i][e] = (overwrite ? 0 : acc[i][e]) + scale * (float)grads[i][e] - one fp32 fused multiply-add per element
 *                          (overwrite: the rounded product).  grads: n_tensors contiguous tensors of `dtype` (FF_DTYPE_F32 / FF_DTYPE_BF16),
 *                          never written; acc: fp32, same sizes.  overwrite != 0 never READS acc (it may hold anything, NaN included): the
 *                          first micro-batch of a step needs no memset pass.  Tensors of any alignment; zero-element tensors are skipped.
 *   ff_adamw_step_acc      ff_adamw_step_mixed / _clipped reading FP32 gradients whatever d->dtype is (the accumulators); grad_coef may be
 *                          NULL (unclipped).  The clip norm over accumulators is ff_grad_sumsq(FF_DTYPE_F32, ...).
 * ------------------------------------------------------------------------------------------------------ */
int ff_grad_accumulate(int dtype, int n_tensors, const void* const* grads, float* const* acc, const long long* numels, float scale,
                       int overwrite, ff_stream_t stream);
int ff_adamw_step_acc(const ff_adamw_desc* d, int state_dtype, void* const* params, const float* const* grads32, void* const* exp_avg,
                      void* const* exp_avg_sq, float* const* master, const float* lr_dev, const float* grad_coef, const long long* numels,
                      ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Non-finite gradients (added under ABI 6): a step whose gradients hold an inf or a NaN is NOT taken - what training under a loss scaler
 * (the reference's `--fp16`, training/train.sh) does - decided and carried out on the device, so that it works inside a replayed HIP graph.
 * Definition: the step is skipped iff the sum of squares of the (grad_scale'd) gradients - fp32 per workgroup (ff_grad_sumsq), fp64 over
 * workgroups (ff_grad_sumsq_reduce) - is non-finite.  Squares are non-negative, so nothing cancels: every inf / NaN element is found; so are
 * finite gradients so large that one 32768-element chunk's sum of squares overflows fp32 (a norm beyond about 1.8e19).
 *   ff_grad_guard          one thread; every pointer is a device scalar.  ff_grad_clip_coef plus the verdict:
 *                            inv   = ext_scale ? 1 / *ext_scale : 1                  (a loss scale the gradients still carry)
 *                            nrm   = (float)sqrt(*sum) * inv                         (*sum read as 0 when sum is NULL: no norm was computed)
 *                            bad   = !isfinite(*sum) || (ext_found_inf && *ext_found_inf != 0) || !isfinite(inv)
 *                            *skip = bad ? 1 : 0;   *take = 1 - *skip;   *norm = nrm (a non-finite value is reported as it is)
 *                            *coef = bad ? 0 : inv * (max_norm > 0 ? min(1, max_norm / (nrm + 1e-6)) : 1);   *skipped_total += bad
 *                          in fp32, each operation rounded once.  sum may be NULL if ext_found_inf is given; ext_found_inf, ext_scale, norm,
 *                          take and skipped_total are optional; coef and skip are required (FF_ERR_SHAPE).  For a finite sum, no ext_*
 *                          arguments and max_norm > 0, *norm and *coef are ff_grad_clip_coef's bit for bit.
 *   ff_adamw_step_guarded  ff_adamw_step_clipped (grads_fp32 == 0) or ff_adamw_step_acc (grads_fp32 != 0: `grads` are fp32 accumulators)
 *                          whose every workgroup reads *skip first and returns before it loads or stores a single tensor element when it is
 *                          != 0: a skipped launch is a no-op - no weight decay, no decay of the moments, no write of the master copies.
 *                          grad_coef and skip are both required.  The caller advances the device step count by *take, not by 1.
 * ------------------------------------------------------------------------------------------------------ */
int ff_grad_guard(const double* sum, float max_norm, const float* ext_found_inf, const float* ext_scale, float* norm, float* coef,
                  float* skip, float* take, long long* skipped_total, ff_stream_t stream);
int ff_adamw_step_guarded(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, int grads_fp32,
                          void* const* exp_avg, void* const* exp_avg_sq, float* const* master, const float* lr_dev, const float* grad_coef,
                          const float* skip, const long long* numels, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Stochastic rounding for pure-bf16 training (added under ABI 6): at lr 1e-4 an update is below half a bf16 ulp of most weights, and a
 * store that rounds to nearest loses it every step.  Here the fp32 result x (bit pattern b) is stored as one of its two bf16 neighbours,
 * the farther one with probability proportional to the distance, so that every store is unbiased:
 *     r = 16 random bits;  s = b + r (32-bit add);  stored = (exponent field of s all ones ? b : s) >> 16
 * (the exception keeps a carry past the largest finite bf16 from producing an infinity); a non-finite x is stored as round-to-nearest
 * stores it.  A representable x is stored unchanged; exactly b & 0xFFFF of the 65536 values of r round away from zero; -0 stays -0.
 * Random bits: Philox4x32 with 7 rounds (Random123's round function and constants), one call per 8-element vector of one stored array:
 *     key     = (seed low 32, seed high 32)
 *     counter = (vec low 32, vec high 32, step, stream_id << 2 | slot)      vec = element index within the tensor >> 3
 *     slot    = 0 parameter, 1 exp_avg, 2 exp_avg_sq;   stream_id < 2^30 names the tensor;   step = the number of the step being taken
 *     element e takes 16 bits of output word (e & 7) >> 1: the low half if e is even, the high half if it is odd
 * so the stored bits do not depend on alignment, on how tensors are grouped into calls, or on the path (vector / element-wise) that ran.
 *   ff_adamw_step_sr          ff_adamw_step_guarded's argument list without `master`, plus the seed (its 64 bits, signedness ignored) and
 *                             one stream id per tensor (a HOST array).  bf16 parameters only (FF_ERR_UNSUPPORTED otherwise); the parameter
 *                             store uses slot 0 and, where state_dtype is bf16, the moment stores slots 1 and 2 (fp32 moments are stored as
 *                             they are).  grad_coef and skip may be NULL: both NULL = ff_adamw_step_mixed's arithmetic (grads_fp32 != 0:
 *                             ff_adamw_step_acc's), grad_coef alone = ff_adamw_step_clipped's, both = ff_adamw_step_guarded's.  step is
 *                             d->step, or *d->step_dev converted to unsigned.  FF_ERR_SHAPE for a null stream_ids or an id >= 2^30.
 *   ff_stochastic_round_bf16  dst[i] (bf16) = src[i] (fp32) by the same rule with the bits of element i: n contiguous elements of any
 *                             alignment, slot 0 .. 3.  The rule on its own (tests), and an unbiased bf16 copy of fp32 weights.
 * ------------------------------------------------------------------------------------------------------ */
int ff_adamw_step_sr(const ff_adamw_desc* d, int state_dtype, void* const* params, const void* const* grads, int grads_fp32,
                     void* const* exp_avg, void* const* exp_avg_sq, const float* lr_dev, const float* grad_coef, const float* skip,
                     long long seed, const unsigned* stream_ids, const long long* numels, ff_stream_t stream);
int ff_stochastic_round_bf16(const float* src, void* dst, long long n, long long seed, unsigned stream_id, unsigned step, int slot,
                             ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Exponential moving average (Polyak average) of the weights (added under ABI 6): an fp32 shadow of every parameter, averaged on the
 * device right after the AdamW launch that wrote the weights, so that a captured step contains it and a step skipped on the device
 * (ff_grad_guard's *skip) leaves it alone.  The rule, in fp32, each operation rounded once, the same code whether the step count comes
 * from the host or from the device:
 *     t    = step_dev ? *step_dev : (float)step                 // number of the step just taken, >= 1
 *     if (skip && *skip != 0) return;                           // wave-uniform, before any tensor access (as GUARD)
 *     if (every > 1 && fmodf(t, (float)every) != 0) return;     // wave-uniform
 *     d_t  = warmup ? fminf(decay, (1.0f + t) / (10.0f + t)) : decay
 *     a    = 1.0f - d_t
 *     th   = master ? master[i][e] : (float)params[i][e]        // bf16 widened exactly
 *     ema[i][e] = fmaf(a, th - ema[i][e], ema[i][e])
 *   ff_ema_update   n_tensors contiguous tensors of any alignment, zero-element tensors skipped, in launches of up to 32 tensors.  dtype:
 *                   the parameters' type (FF_DTYPE_F32 / FF_DTYPE_BF16).  master: fp32 master copies or NULL; where it is given, params is
 *                   not read and may be NULL.  ema: the fp32 shadows (always fp32: a bf16 shadow rounded to nearest never moves at decay
 *                   0.9999, a stochastically rounded one carries a standing error of about 29 ulps - DESIGN.md).  step_dev and skip are
 *                   device scalars or NULL.  FF_ERR_SHAPE before any HIP call: decay outside (0, 1), every < 1, step < 1 without
 *                   step_dev, a null table with n_tensors > 0.  n_tensors == 0 is FF_OK.
 * ------------------------------------------------------------------------------------------------------ */
int ff_ema_update(int dtype, int n_tensors, const void* const* params, const float* const* master, float* const* ema,
                  const long long* numels, float decay, int warmup, int every, int step, const float* step_dev,
                  const float* skip, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Shifted next-token cross-entropy (modeling_flamingo.py:288-298): position i predicts labels[i+1].
 * logits (batch, seq, vocab) contiguous; labels (batch, seq) int64; rows = batch * (seq - 1).
 * fwd: loss_row[r] = logsumexp(logits[b,i,:]) - logits[b,i,labels[b,i+1]] (0 where the label == ignore_index), lse[r] saved.
 * bwd: dlogits[b,i,:] = (softmax - onehot) * grad_row[r];  dlogits[b,seq-1,:] = 0.   The reduction (mean over the
 * non-ignored rows / sum / none) is applied by the caller on the `rows` values.
 * ------------------------------------------------------------------------------------------------------ */
int ff_shifted_ce_fwd(int dtype, int batch, int seq, int vocab, const void* logits, const long long* labels, long long ignore_index,
                      float* loss_row, float* lse, ff_stream_t stream);
int ff_shifted_ce_bwd(int dtype, int batch, int seq, int vocab, const void* logits, const long long* labels, long long ignore_index,
                      const float* lse, const float* grad_row, void* dlogits, ff_stream_t stream);
/* Label smoothing and z-loss in the same two passes (added under ABI 6).  eps = label_smoothing in [0, 1], zeta = z_loss >= 0 and finite;
 * anything else (NaN included) returns FF_ERR_UNSUPPORTED before any launch.  Per scored row, fp32 math on the logits x as stored:
 *   fwd: lse[r] as above, unchanged;   loss_row[r] = lse - (1 - eps) x_t - eps mean_c(x_c) + zeta lse^2
 *        (zeta = 0: F.cross_entropy(label_smoothing=eps) on the shifted logits and labels, HF LabelSmoother(epsilon=eps))
 *   bwd: dlogits[b,i,c] = grad_row[r] * (p_c (1 + 2 zeta lse) - (1 - eps) [c == t] - eps / vocab),   p_c = exp(x_c - lse)
 * Ignored rows (loss 0, gradient row exactly 0), the last position (gradient row exactly 0) and a label outside [0, vocab) (NaN loss, NaN
 * row, nothing read out of bounds) are as in the plain entry points.  -inf logits are as in torch: with eps > 0 the row's loss is +inf
 * (the mean of -log p is), its gradient stays finite, -eps / vocab * grad_row at the -inf columns; with eps = 0 everything stays finite.
 * No atomics: the same bits on every run.  With eps = 0 and zeta = 0 the plain kernels are launched: the bits of ff_shifted_ce_fwd/bwd.
 * The two values are launch constants: a captured graph keeps the ones it was captured with. */
int ff_shifted_ce_fwd_reg(int dtype, int batch, int seq, int vocab, const void* logits, const long long* labels, long long ignore_index,
                          float* loss_row, float* lse, float label_smoothing, float z_loss, ff_stream_t stream);
int ff_shifted_ce_bwd_reg(int dtype, int batch, int seq, int vocab, const void* logits, const long long* labels, long long ignore_index,
                          const float* lse, const float* grad_row, void* dlogits, float label_smoothing, float z_loss, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Token selection for sampled decoding (added under ABI 6): temperature, top-k and nucleus (top-p) filtering and the draw, one launch, no
 * sort, no random-number generation (the caller supplies the uniform numbers), capturable.
 * logits: `rows` rows of `vocab` elements of `dtype` (FF_DTYPE_F32 / FF_DTYPE_BF16), row r at element r * ld, ld >= vocab; rows need only
 * element alignment (logits[:, -1] of a (batch, seq, vocab) tensor: ld = seq * vocab).  u: rows fp32 values in [0, 1).  token: rows int64.
 * Per row, x_i the logits as stored:
 *   1. K = {i : x_i >= the top_k-th largest x}: ties with that value are all kept.   top_k == 0 or >= vocab: every i.
 *   2. z_i = x_i / temperature,  q_i = exp(z_i - max z) / sum_{j in K} exp(z_j - max z).
 *   3. P = {i in K : sum of q_j over the j in K with x_j > x_i (strictly) < top_p}: equal values stay or go together, the maximum always
 *      stays.   top_p == 1: P = K.
 *   4. S = sum_{i in P} q_i; token = the smallest i in P whose inclusive prefix sum over P, in index order, exceeds u * S (the last element
 *      of P if rounding leaves none).
 * -inf logits (masked entries) are never chosen.  A row that holds a NaN or +inf, or nothing but -inf, gives an unspecified token inside
 * [0, vocab).  fp32 math in a fixed order: equal inputs give equal tokens, eager or replayed from a graph.
 * FF_ERR_SHAPE: a null pointer, rows <= 0, vocab <= 0, ld < vocab, temperature not positive and finite, top_k < 0, top_p outside (0, 1].
 * ------------------------------------------------------------------------------------------------------ */
int ff_sample_token(int dtype, int rows, int vocab, long long ld, const void* logits, float temperature, int top_k, float top_p,
                    const float* u, long long* token, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Token selection under the truncation samplers (added under ABI 6): ff_sample_token's filters followed by min_p, typical_p,
 * epsilon_cutoff and eta_cutoff - transformers' MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper (each with
 * min_tokens_to_keep = 1), in transformers' order - and the draw, one launch, no sort, capturable.  logits, ld, u and token are as in
 * ff_sample_token.  Per row, x_i the logits as stored, z_i = x_i / temperature; "q renormalised over a set" is exp(z_i - max z) divided
 * by its sum over that set:
 *   1. K0 = rule 1 of ff_sample_token (top-k).
 *   2. K1 = rule 3 of ff_sample_token (the nucleus within K0).
 *   3. min_p:  K2 = {i in K1 : exp(z_i - max z) >= min_p}, i.e. q_i >= min_p * max q.   min_p == 0: K2 = K1.
 *   4. typical_p:  r = q renormalised over K2, H = -sum_{K2} r log r, d_i = |-log r_i - H|;
 *      K3 = {i in K2 : sum of r_j over the j in K2 with d_j < d_i (strictly) < typical_p}.   typical_p == 1: K3 = K2.
 *   5. epsilon_cutoff:  r = q renormalised over K3;  K4 = {i in K3 : r_i >= epsilon_cutoff, or x_i is the largest value of K3}.
 *      epsilon_cutoff == 0: K4 = K3.
 *   6. eta_cutoff:  r and H over K4, eta* = min(eta_cutoff, sqrt(eta_cutoff) * exp(-H));
 *      K5 = {i in K4 : r_i >= eta*, or x_i is the largest value of K4}.   eta_cutoff == 0: K5 = K4.
 *   7. S = sum over K5 of q; token = the smallest i in K5 whose inclusive prefix sum over K5, in index order, exceeds u * S (the last
 *      element of K5 if rounding leaves none): rule 4 of ff_sample_token over K5.
 * Every stage is a function of the value: equal values stay or go together, every stage keeps all columns of its largest kept value, so K5
 * is never empty.  -inf logits are never chosen.  A row that holds a NaN or +inf, or nothing but -inf, gives an unspecified token inside
 * [0, vocab).  fp32 math in a fixed order: equal inputs give equal tokens, eager or replayed from a graph.  The four values are launch
 * constants.  With all four off the result is ff_sample_token's.
 * FF_ERR_SHAPE: what ff_sample_token rejects; min_p outside [0, 1], typical_p outside (0, 1], epsilon_cutoff or eta_cutoff outside [0, 1),
 * any of them not finite.  FF_ERR_UNSUPPORTED: another dtype.
 * ------------------------------------------------------------------------------------------------------ */
int ff_sample_token_truncated(int dtype, int rows, int vocab, long long ld, const void* logits, float temperature, int top_k, float top_p,
                              float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff, const float* u, long long* token,
                              ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Beam search on the captured decode step (added under ABI 6): ff_beam_step selects and keeps ALL bookkeeping on the device (no host
 * synchronisation, no allocation), ff_beam_gather reorders the static LM cache in place.  Both are capturable.
 * logits: rows = b * nb rows of `vocab` elements of `dtype`, row r at element r * ld, ld >= vocab, element alignment only; row s * nb + k
 * is beam k of sequence s.  cur_len: a device int64, the length the sequences have AFTER this step's token (1 <= *cur_len <= max_len).
 * The state block belongs to the caller, who initialises it once (score[s][0] = 0, every other score -inf, done / n_hyp 0) and fills
 * len_norm[t] = float32(t ** length_penalty), t = 0 .. max_len; after that only the library writes it:
 *   score[b][nb] fp32 (-inf = a dead beam), done[b], n_hyp[b] int32, finished hypotheses hyp_score / hyp_len / hyp_row [b][nb] (sorted by
 *   score, best first), histories hist_tok int64 / hist_parent int32 / hist_score fp32 [max_len][b * nb], and the step's results
 *   next_tok[b * nb] int64 and beam_idx[b * nb] int64 (GLOBAL row indices: the argument of ff_beam_gather).
 * Rules (FlamingoModel._beam_search, step for step), per sequence s:
 *   1. per row  lse = max + log(sum exp(x - max))  in fp32, in a fixed summation order;
 *   2. logp_v = x_v - lse;
 *   3. candidate (k, v) scores  score[s][k] + logp_v,  each operation rounded once in fp32;
 *   4. the 2 nb best candidates are taken, ordered by score descending, then by flat index k * vocab + v ascending (ties are decided);
 *   5. a -inf candidate is taken only if fewer finite ones exist;
 *   6. the ranks are walked in order until nb beams are filled: an eos candidate at rank < nb becomes a finished hypothesis
 *      (score / len_norm[*cur_len] in fp32, *cur_len, parent row), at rank >= nb it is dropped; the first nb other candidates become the next
 *      beams (missing ones: -inf, pad, the identity parent); hypotheses are kept sorted, equal scores in arrival order, the best nb stay; with
 *      nb of them, done[s] is set if early_stopping, or if the worst kept one >= (best next score) / len_norm[*cur_len].  A sequence that was
 *      done before the call gets -inf, pad and the identity parent and keeps its hypotheses;
 *   7. token, parent row and score of every row go into the history tables at index *cur_len - 1 (a hypothesis or an open beam is read
 *      back by following hist_parent downwards from its row);
 *   8. a row holding NaN or +inf gives unspecified candidates, but every index written stays in range;
 *   9. fixed order throughout: equal inputs give equal bits, eager or replayed.
 * eos = -1: none.  workspace: ff_beam_workspace_bytes(b, nb) bytes (0 for arguments ff_beam_step rejects).
 * FF_ERR_SHAPE: a null pointer, b <= 0, nb outside [1, FF_BEAM_MAX], vocab < 2 nb, ld < vocab, max_len < 1, a workspace that is too small.
 * FF_ERR_UNSUPPORTED: other dtypes.
 *
 * ff_beam_gather: t[row, o, p, :] <- t[beam_idx[row], o, p, :] for every tensor of the table (host array of n_tensors device pointers, each
 * (b * nb, outer, len_max, inner) contiguous, elements of elem_size 2 or 4 bytes) and every position p < *n_pos (a device int64, clamped to
 * [0, len_max]); positions >= *n_pos are neither read nor written.  beam_idx[row] must lie in the nb rows of row's sequence (otherwise the
 * row stays) and may repeat a row.  In place: one thread moves one 16-byte vector (or element, when inner * elem_size or a pointer is not a
 * multiple of 16) of all nb rows of a sequence, loads before stores.  FF_ERR_SHAPE: null pointers, non-positive sizes, nb outside
 * [1, FF_BEAM_MAX]; FF_ERR_UNSUPPORTED: another element size.
 * (ff_beam_desc is declared struct-then-typedef; tests/test_beam_args.py checks its ctypes mirror against this header.)
 * ------------------------------------------------------------------------------------------------------ */
#define FF_BEAM_MAX 8
struct ff_beam_desc {
    int dtype, b, nb, vocab;
    long long ld;
    int max_len, eos, pad, early_stopping;
    float* score;
    int* done;
    int* n_hyp;
    float* hyp_score;
    int* hyp_len;
    int* hyp_row;
    long long* hist_tok;
    int* hist_parent;
    float* hist_score;
    long long* next_tok;
    long long* beam_idx;
    const float* len_norm;
};
typedef struct ff_beam_desc ff_beam_desc;
size_t ff_beam_workspace_bytes(int b, int nb);
int ff_beam_step(const ff_beam_desc* d, const void* logits, const long long* cur_len, void* workspace, size_t workspace_bytes,
                 ff_stream_t stream);
int ff_beam_gather(int n_tensors, void* const* tensors, int elem_size, int b, int nb, long long outer, long long len_max, long long inner,
                   const long long* beam_idx, const long long* n_pos, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Diverse beam search (Vijayakumar et al.) on the captured decode step (added under ABI 6): ff_group_beam_step is ff_beam_step with the nb
 * beams of a sequence split into G = n_groups groups of gs = nb / G; the rows of group g are s * nb + g * gs + j, j < gs.  Inside a step the
 * groups are handled in the order g = 0 .. G - 1, and a group pays diversity_penalty (lambda) for every token an earlier group chose in this
 * step.  ff_beam_desc is unchanged: done and n_hyp hold b * G entries ([b][G]), hyp_score / hyp_len / hyp_row [b][nb] are read as
 * [b][G][gs]; every other field and the workspace (ff_beam_workspace_bytes) are those of ff_beam_step.  The caller initialises score to 0 for
 * beam 0 OF EVERY GROUP and to -inf for every other beam.  Capturable: no allocation, no host synchronisation, fixed order.  Rules:
 *   A. the score of token v on row r of group g is  fl(fl(fl(x_v - lse_r) + score_r) - fl(lambda * c_g(v))),  each operation rounded once in
 *      fp32; the row part is rules 1 - 3 above.  c_g(v) = the number of rows of groups 0 .. g - 1 of the same sequence whose NEXT beam of this
 *      step is live (new score > -inf) and carries token v; dead rows and the rows of a done group hold pad and count nothing.  With c = 0
 *      nothing is subtracted: no bit changes;
 *   B. inside group g rules 4 - 7 apply with nb replaced by gs: the 2 gs best of the group's gs * vocab candidates, score descending, then row,
 *      then column ascending; eos at rank < gs becomes a hypothesis of THAT group, at a later rank it is dropped; every group has its own sorted
 *      list of gs hypotheses, its own n_hyp and done, its own early-stopping test; the rows of a done group get -inf, pad and the identity
 *      parent.  The PENALISED score is the beam's running score and the hypothesis' score: penalties accumulate over the steps, as in the
 *      published algorithm, so scores under groups are not pure log-probabilities;
 *   F. rule 8 holds: whatever a row contains, every index written stays inside its table.
 * n_groups = 1 is ff_beam_step: the same two launches, the same bits.  n_groups > 1 with lambda = 0 makes every group an independent
 * ff_beam_step of gs beams on its rows.  (A row's 2 gs best penalised candidates lie among its 2 nb best unpenalised ones - the penalty lowers
 * at most nb - gs columns -, so the row pass of ff_beam_step serves unchanged and the group walk is one launch of one wave per sequence.)
 * FF_ERR_SHAPE: n_groups < 1, nb not a multiple of n_groups, a negative or non-finite diversity_penalty, and everything ff_beam_step rejects.
 * ------------------------------------------------------------------------------------------------------ */
int ff_group_beam_step(const ff_beam_desc* d, int n_groups, float diversity_penalty, const void* logits, const long long* cur_len,
                       void* workspace, size_t workspace_bytes, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Beam sampling (transformers' beam-sample: num_beams > 1 with do_sample) on the captured decode step (added under ABI 6):
 * ff_beam_sample_step is ff_beam_step with its rule 4 replaced by a DRAW.  As in current transformers (_get_top_k_continuations) the warpers
 * act on each row's log-probabilities, the beam's running score is added, 2 nb continuations are drawn WITHOUT replacement from the softmax
 * over the sequence's nb * vocab accumulated scores, and the drawn ones are sorted by accumulated score and walked as in plain beam search.
 * The draw is a Gumbel top-k: the 2 nb largest values of a + g, g i.i.d. standard Gumbel noise, have exactly the law of
 * torch.multinomial(softmax(a), 2 nb, replacement=False) - the Plackett-Luce law (Kool et al., "Stochastic Beams and Where to Find Them",
 * 2019, section 3).  ff_beam_desc, the state block and its initialisation are those of ff_beam_step.  seed: a device int64.
 * Per sequence s, row r = s * nb + k, x the logits as stored:
 *  S1. lse_r and logp_v = x_v - lse_r, exactly as rules 1 - 2 of ff_beam_step.
 *  S2. the warpers, per row, in transformers' order, by the value rules of ff_sample_token: K = its rule 1 (top-k by value, ties all kept),
 *      P = its rule 3 (the nucleus over q = softmax(logp / T) within K; equal values stay or go together, the maximum always stays);
 *      z_v = logp_v / T for v in P, -inf otherwise, rounded once.  Nothing is renormalised, as in transformers.  With T = 1, top_k = 0 and
 *      top_p = 1, z_v is logp_v bit for bit.
 *  S3. a(k, v) = fl(z_v + score[s][k]).  With the warpers off this is ff_beam_step's candidate score, bit for bit.
 *  S4. the noise: w = word v & 3 of Philox4x32-7 (Random123's round function, 7 rounds) with key (seed low 32 bits, seed high 32 bits) and
 *      counter (v >> 2, r, (unsigned)*cur_len, 0x42534D50);  u = ((w >> 9) + 0.5) * 2^-23, exact in fp32 and inside [2^-24, 1 - 2^-24];
 *      g = -logf(-logf(u)).  Nothing of the launch geometry enters: eager and replayed steps draw the same numbers whatever the grid.
 *  S5. p(k, v) = fl(a + g).  The sequence's candidates are the 2 nb largest p, ordered by p descending, then by flat index k * vocab + v
 *      ascending.  A candidate with a = -inf (a filtered token, a dead beam, a masked logit) has p = -inf and is taken only if fewer finite
 *      ones exist (rule 5), lowest flat index first.
 *  S6. the 2 nb candidates are ordered by a descending, then by flat index ascending, and rules 6 - 9 of ff_beam_step apply to them
 *      unchanged: hypotheses, done, the history tables, next_tok, beam_idx.  Running and hypothesis scores are a, never p.
 * Known and accepted: with top_k < 2 nb the first step has fewer than 2 nb finite candidates and the missing beams are dead.  The law of the
 * draw is truncated at |g| ~ 16.6 (the 23-bit grid of u), which has probability about 6e-8 per entry.
 * Capturable: two launches, no allocation, no host synchronisation, no global atomics, a fixed order - equal inputs and an equal seed give
 * equal bits.  temperature, top_k and top_p are launch constants.  workspace: ff_beam_sample_workspace_bytes(b, nb) bytes (0 for arguments
 * the step rejects).  After the call it holds what the rows handed the merge, for inspection: p [b * nb][2 nb] fp32, then a [b * nb][2 nb]
 * fp32, then the column [b * nb][2 nb] int32 - each row's best 2 nb candidates by (p, column); with nb = 1 that is the sequence's draw.
 * ff_beam_sample_noise writes g of rule S4 for rows 0 .. rows - 1 and columns 0 .. vocab - 1 into a (rows, vocab) fp32 buffer, rows <= 65535:
 * the hook that ties the kernels' noise to a restatement.
 * FF_ERR_SHAPE: everything ff_beam_step rejects; temperature, top_k, top_p as ff_sample_token rejects them; a null seed.
 * FF_ERR_UNSUPPORTED: other dtypes.
 * ------------------------------------------------------------------------------------------------------ */
size_t ff_beam_sample_workspace_bytes(int b, int nb);
int ff_beam_sample_step(const ff_beam_desc* d, float temperature, int top_k, float top_p, const long long* seed, const void* logits,
                        const long long* cur_len, void* workspace, size_t workspace_bytes, ff_stream_t stream);
int ff_beam_sample_noise(int rows, int vocab, const long long* seed, const long long* cur_len, float* g, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Contrastive search (Su et al. 2022, "A Contrastive Framework for Neural Text Generation"; transformers' penalty_alpha with top_k) on the
 * captured decode step (added under ABI 6): ff_topk_logprob lists a row's k best tokens with their log-probabilities, ff_contrastive_step
 * ranks the k candidates of every sequence by model confidence minus their similarity to the context, chooses one and keeps the
 * bookkeeping on the device.  Both are capturable: no allocation, no host synchronisation, no global atomics.
 * Per sequence s, with n tokens so far (prompt included) and H[s, j] the lm_head input at position j < n:
 *   T.  candidates: from the step's logits (after the processors and constraints) the k largest VALUES, ordered by value descending, then by
 *       index ascending; they are compared as values, so the tokens are exact.  logp = x - lse in fp32, lse as in rules 1 - 2 of
 *       ff_beam_step.  A -inf logit is listed only if fewer than k finite ones exist: a DEAD candidate, logp = -inf, its token unspecified but
 *       in range;
 *   C1. every candidate c is fed to the LM as the next token - k rows per sequence that share the sequence's cache -, which gives h_c (the
 *       lm_head input) and the next logits.  (The caller's part.)
 *   C2. cos_cj = <h_c, H_sj> / (max(|h_c|, 1e-12) * max(|H_sj|, 1e-12)), in fp32 in a fixed order, over the j < n with mask[s, j] != 0 (left
 *       padding of the prompt is excluded, as in transformers);
 *   C3. pen_c = max_j cos_cj; 0 if no live position exists;
 *   C4. score_c = (1 - alpha) * exp(logp_c) - alpha * pen_c; a dead candidate scores -inf;
 *   C5. c* = the smallest c of maximal score; 0 if every candidate is dead;
 *   C6. a sequence that had finished gets pad and log-probability 0; otherwise the token is candidate c*'s, its log-probability logp_c*, and
 *       finished |= token == eos;
 *   C7. the state advances for every sequence, finished or not: H[s, n] <- h_c* (bit for bit), and the chosen row's cache and next logits
 *       become the sequence's: sel_row[s] = s * k + c*, and beam_idx[s * k + i] = sel_row[s] for every i < k is the argument of ff_beam_gather;
 *   C8. a row holding NaN or +-inf gives an unspecified choice, but every index written stays in range;
 *   C9. fixed order throughout: equal inputs give equal bits, eager or replayed.
 * Deliberate deviation from transformers: there a banned token (probability 0) can win on its penalty alone and a zero vector gives NaN;
 * here dead candidates never win and the norms are clamped.
 * ff_topk_logprob: logits are rows of `vocab` elements of `dtype` (bf16 or fp32), row r at element r * ld, ld >= vocab, element alignment
 * only; tok [rows][k] int64 and logp [rows][k] fp32 are written; 1 <= k <= FF_CONTRASTIVE_K_MAX.  One launch, one workgroup per row.
 * FF_ERR_SHAPE: a null pointer, rows <= 0, vocab <= 0, ld < vocab, k outside [1, FF_CONTRASTIVE_K_MAX], vocab < k.  FF_ERR_UNSUPPORTED: other dtypes.
 * ff_contrastive_step: rules C2 - C7 in one launch, one workgroup per sequence (no workgroup waits for another).  hidden: [b * k][dim] of
 * `dtype`, row r at element r * ld_hidden; hist: [b][max_len][dim] of `dtype`, contiguous, read at positions < *n_pos and written at
 * *n_pos (nowhere if *n_pos is outside [0, max_len)); mask [b][max_len] uint8; cand_tok int64 / cand_logp fp32 [b][k] (what ff_topk_logprob
 * wrote for the rows the candidates came from); finished [b] uint8, read and written; outputs next_tok [b] int64, logprob [b] fp32, sel_row
 * [b] int64, beam_idx [b * k] int64, and - optional, may be NULL - score [b][k] fp32, the values of rule C4, for inspection.  eos = -1:
 * none.  alpha and n_pos (= n) are DEVICE scalars: a captured call serves every value written there.  The workgroup keeps the k candidate
 * vectors in LDS and reads H[s, :n] once.
 * FF_ERR_SHAPE: a null pointer (score excepted), b, dim or max_len <= 0, k outside [1, FF_CONTRASTIVE_K_MAX], ld_hidden < dim.
 * FF_ERR_UNSUPPORTED: other dtypes; k * dim * sizeof(element) > 131072 bytes (k = 8 serves dim <= 4096 in both dtypes).
 * (ff_contrastive_desc is declared struct-then-typedef, like ff_beam_desc.)
 * ------------------------------------------------------------------------------------------------------ */
#define FF_CONTRASTIVE_K_MAX 8
struct ff_contrastive_desc {
    int dtype, b, k, dim;
    long long ld_hidden;
    int max_len, eos, pad, reserved;
    const void* hidden;
    void* hist;
    const unsigned char* mask;
    const long long* cand_tok;
    const float* cand_logp;
    unsigned char* finished;
    long long* next_tok;
    float* logprob;
    long long* sel_row;
    long long* beam_idx;
    float* score;
};
typedef struct ff_contrastive_desc ff_contrastive_desc;
int ff_topk_logprob(int dtype, int rows, int vocab, long long ld, const void* logits, int k, long long* tok, float* logp, ff_stream_t stream);
int ff_contrastive_step(const ff_contrastive_desc* d, const float* alpha, const long long* n_pos, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Logits processors on the captured decode step (added under ABI 6): repetition penalty, no-repeat n-gram ban and minimum length, applied
 * IN PLACE to the rows a step is about to select from (argmax, ff_sample_token, ff_beam_step).  One launch, no allocation, no host
 * synchronisation, capturable; equal inputs give equal bits, eager or replayed.
 * logits: `rows` rows of `vocab` elements of `dtype` (FF_DTYPE_F32 / FF_DTYPE_BF16), row r at element r * ld, ld >= vocab, element alignment
 * only (the contract of ff_sample_token: logits[:, -1] of a (batch, seq, vocab) tensor works).  hist: int64 token ids, row r at
 * hist + r * hist_ld, hist_ld >= hist_cap.  *hist_len: a device int64, the number of tokens the sequences already hold, one value for all
 * rows, clamped to [0, hist_cap]: n.  Positions >= n of hist are never read.  *min_len: a device int64; min_len may be null.
 * Rules, per row; h = the row's first n history tokens, x = the row's logits as stored:
 *   1. repetition penalty p, applied when p != 1: once for every DISTINCT token t in h with 0 <= t < vocab - a token that occurs several
 *      times is still penalised exactly once - x_t becomes  x_t < 0 ? x_t * p : x_t * rp,  rp = 1.0f / p computed once on the host in
 *      fp32; the product is computed in fp32 and rounded once to the dtype, round to nearest even.  (transformers divides where this
 *      multiplies by the reciprocal: the results differ by at most one fp32 ulp, and this one is reproducible bit for bit.)  A NaN x_t
 *      keeps its bits.
 *   2. no-repeat n-gram of size g, applied when g >= 1 and n >= g: for every i in [0, n - g] with h[i .. i+g-2] == h[n-g+1 .. n-1] the
 *      token h[i+g-1] gets -inf, if it lies in [0, vocab).  With g = 1 every token of h is banned.  Tokens outside [0, vocab) still take
 *      part in the comparisons.
 *   3. minimum length: if eos >= 0, min_len is not null and n < *min_len, x_eos = -inf.
 *   4. bans win over the penalty.  Every entry not named above keeps its bits; NaN stays NaN under the penalty; nothing outside
 *      [0, vocab) of a row is written.
 * With p == 1, g == 0 and rule 3 off (eos < 0 or min_len null) the call returns FF_OK and launches nothing.
 * FF_ERR_SHAPE: null logits, hist or hist_len; rows <= 0, vocab <= 0, ld < vocab; hist_cap < 1, hist_ld < hist_cap; p not positive and
 * finite; g < 0; eos outside [-1, vocab).  FF_ERR_UNSUPPORTED: another dtype, hist_cap > FF_LOGITS_HIST_MAX.
 * ------------------------------------------------------------------------------------------------------ */
#define FF_LOGITS_HIST_MAX 4096
int ff_logits_process(int dtype, int rows, int vocab, long long ld, void* logits,
                      const long long* hist, long long hist_ld, long long hist_cap, const long long* hist_len,
                      float repetition_penalty, int no_repeat_ngram_size, int eos, const long long* min_len,
                      ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Log-probability of a chosen token (added under ABI 6): logprob[r] = x_tok - logsumexp(x) for the rows a decode step just selected
 * from.  One launch, no atomics, no allocation, no host synchronisation, capturable; equal inputs give equal bits, eager or replayed.
 * logits: `rows` rows of `vocab` elements of `dtype` (FF_DTYPE_F32 / FF_DTYPE_BF16), row r at element r * ld, ld >= vocab, element alignment
 * only (the contract of ff_sample_token: logits[:, -1] of a (batch, seq, vocab) tensor works in place); never written.  token: rows int64.
 * skip: rows bytes, or null.  logprob: rows fp32.  lse: rows fp32, or null.
 * Per row, fp32 math in the order of ff_shifted_ce_fwd (one 256-thread workgroup, (max, sum) pairs, a fixed wave and block combine,
 * lse = M + logf(S)): for a row at the same address lse has the bits ff_shifted_ce_fwd stores, and logprob == -loss_row bit for bit.
 *   logprob[r] = x_tok - lse, and lse[r] = lse when lse is not null;
 *   token[r] outside [0, vocab): logprob[r] = NaN, nothing is read out of bounds;
 *   x_tok == -inf: -inf; -inf at other columns contributes 0; a row holding NaN or +inf: NaN;
 *   skip[r] != 0: logprob[r] = 0 and lse[r] = 0 exactly, the row is not read.
 * FF_ERR_SHAPE: null logits, token or logprob; rows <= 0, vocab <= 0, ld < vocab.  FF_ERR_UNSUPPORTED: another dtype.  Both before any
 * launch.
 * ------------------------------------------------------------------------------------------------------ */
int ff_token_logprob(int dtype, int rows, int vocab, long long ld, const void* logits, const long long* token, const unsigned char* skip,
                     float* logprob, float* lse, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Constrained decoding on the captured decode step (added under ABI 6): a trie of candidate sequences and a list of banned words, applied
 * IN PLACE to the rows a step is about to select from (argmax, ff_sample_token, ff_beam_step), after ff_logits_process.  The rules only
 * ever write -inf.  One launch, no allocation, no host synchronisation, no global atomics, capturable; equal inputs give equal bits, eager
 * or replayed.  Everything the kernel reads about the constraint lives in device memory, with CAPACITIES fixed at launch and live SIZES
 * read on the device: one captured launch serves every candidate set and word list that fits the capacities.
 * logits, hist, hist_ld, hist_cap, *hist_len: the contract of ff_logits_process (row r at element r * ld, ld >= vocab, element alignment
 * only; int64 ids; *hist_len clamped to [0, hist_cap]: n; positions >= n are never read).  *gen_start: a device int64, clamped to
 * [0, n]: n0, the position at which the generated tokens begin.  h = the row's first n tokens, g = h[n0 .. n), x = the row's logits.
 * Trie (root = node 0) in CSR form: node_first[node_cap + 1] int32 - the edges of node s are node_first[s] .. node_first[s + 1] - ;
 * edge_tok[edge_cap] int32, ascending and distinct inside a node; edge_child[edge_cap] int32; node_terminal[node_cap] bytes (non-zero: a
 * candidate ends here); *n_nodes a device int32, clamped to [0, node_cap].  Entries beyond the live sizes (nodes >= *n_nodes, edges >=
 * node_first[*n_nodes]) are never read.  *n_nodes == 0: the trie rule does nothing.
 *   T1 (position).  s = root.  For each t in g, in order: s DONE or DEAD stays; t == eos and terminal(s): DONE; t is a child token of s:
 *      that child; otherwise DEAD.  (A child token outside [0, vocab) still takes part.)
 *   T2 (mask).  If s is a node, every x_v, v in [0, vocab), with v neither a child token of s nor eos when terminal(s), becomes -inf - a
 *      banned NaN like any entry; every other entry keeps its bits.  If s is DONE or DEAD the trie rule leaves the row UNTOUCHED (an
 *      all -inf row would give ff_beam_step an lse of -inf and NaN candidates; a dead beam already carries the score -inf).
 * Bad words: bw_off[bw_cap + 1] int32 - word w is bw_tok[bw_off[w] .. bw_off[w + 1]) -, bw_tok[bw_tok_cap] int32, *n_bw a device int32,
 * clamped to [0, bw_cap].
 *   B1.  For each word w of length m >= 1, against the WHOLE history h, prompt included (as transformers does): m == 1: x[w_0] = -inf;
 *      m > 1: if n >= m - 1 and h[n-m+1 .. n) == w[0 .. m-1) then x[w_{m-1}] = -inf.  A last token outside [0, vocab) names no logit;
 *      earlier tokens outside the range still take part in the comparison.  A word of length 0 does nothing.
 * The bans of T2 and B1 union.  Nothing outside [0, vocab) of a row is written.  A row left with nothing but -inf gives what
 * ff_sample_token and ff_beam_step document for it: unspecified but in range.  Offsets and child indices that point outside the capacities
 * are clamped or end the walk: a malformed table gives unspecified bans but no access outside the capacities.
 * Either table may be absent (all of its pointers null); with both absent the call returns FF_OK and launches nothing.
 * FF_ERR_SHAPE: null logits, hist, hist_len or gen_start; a table given in part; rows <= 0, vocab <= 0, ld < vocab; hist_cap < 1, hist_ld <
 * hist_cap; a capacity of a given table < 1; eos outside [0, vocab) with a trie, outside [-1, vocab) without one.  FF_ERR_UNSUPPORTED:
 * another dtype, hist_cap > FF_LOGITS_HIST_MAX, vocab > FF_CONSTRAIN_VOCAB_MAX (the allowed set is a vocab-bit bitmap in 32 KiB of LDS).
 * All before any launch.
 * ------------------------------------------------------------------------------------------------------ */
#define FF_CONSTRAIN_VOCAB_MAX 262144
int ff_logits_constrain(int dtype, int rows, int vocab, long long ld, void* logits,
                        const long long* hist, long long hist_ld, long long hist_cap, const long long* hist_len, const long long* gen_start, int eos,
                        const int* node_first, const int* edge_tok, const int* edge_child, const unsigned char* node_terminal, const int* n_nodes,
                        int node_cap, int edge_cap,
                        const int* bw_off, const int* bw_tok, const int* n_bw, int bw_cap, int bw_tok_cap,
                        ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Classifier-free guidance on the captured decode step (added under ABI 6): the scores a step selects from, out of the logits of the same
 * sequence decoded WITH its media (cond) and WITHOUT (uncond):  out = lu + g (lc - lu),  lc / lu the log-softmax of the two rows
 * (transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor).  One launch in front of ff_logits_process, ff_logits_constrain and the
 * selection; no atomics, no allocation, no host synchronisation, capturable; equal inputs give equal bits, eager or replayed.
 * cond, uncond: `rows` rows of `vocab` elements of `dtype` (FF_DTYPE_F32 / FF_DTYPE_BF16), row r at element r * ld_cond resp. r * ld_uncond,
 * every ld >= vocab, element alignment only and independent of each other (the two halves of one (2 rows, vocab) buffer, logits[:, -1] of a
 * (batch, seq, vocab) tensor work in place).  scale: ONE fp32 in DEVICE memory, g, read by the launch: a captured launch serves every g.
 * out: rows of `vocab` fp32, row r at element r * ld_out, element alignment only; it must not overlap the inputs.
 *   G1.  lse_c, lse_u: each row's logsumexp in fp32, the max-shifted (max, sum) pairs from (-FLT_MAX, 0) of ff_shifted_ce_fwd /
 *        ff_token_logprob with their wave and block combine, lse = M + logf(S) (each row walked on its own 16-byte grid).
 *   G2.  lc = x_c - lse_c, lu = x_u - lse_u, out = fmaf(g, lc - lu, lu).  g = 1: the conditional log-softmax; g = 0: the unconditional one.
 *   G3.  x_c == -inf or x_u == -inf: out = -inf, for every g (never the +inf or NaN of (1 - g) * (-inf)).  A row pair in which either row
 *        holds NaN or +inf: the whole out row is NaN (this rule goes first).  A row of nothing but -inf: all -inf.
 *   G4.  Neither input is written; nothing outside out[r, 0 .. vocab) is written.
 * g itself is not checked on the device (NaN or infinite g: unspecified values, in bounds).
 * FF_ERR_SHAPE: null cond, uncond, scale or out; rows <= 0, vocab <= 0, an ld < vocab.  FF_ERR_UNSUPPORTED: another dtype.  Both before any
 * launch.
 * ------------------------------------------------------------------------------------------------------ */
int ff_guided_logits(int dtype, int rows, int vocab, long long ld_cond, const void* cond, long long ld_uncond, const void* uncond,
                     const float* scale, float* out, long long ld_out, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Log-probabilities of many queried tokens per row (added under ABI 6): what FlamingoModel.score_candidates reads from the logits of one
 * level of the candidate trie.  logits follows the contract of ff_token_logprob: `rows` rows of `vocab` elements of `dtype` (FF_DTYPE_F32 /
 * FF_DTYPE_BF16), row r at element r * ld, ld >= vocab, element alignment only (logits[:, -1] of a (rows, 1, vocab) or (rows, 2, vocab)
 * tensor is read in place); never written.  row_first: rows + 1 int32 on the device, a CSR table over the rows - row r owns the queries q
 * in [row_first[r], row_first[r + 1]).  tok: n_q int32 on the device.  base: rows fp32 on the device, or null.  out: n_q fp32 on the
 * device, out[q] belongs to query q.
 *   S1.  lse_r is computed with ff_token_logprob's row pass, operation for operation (one 256-thread workgroup per row, (max, sum) pairs
 *        from (-FLT_MAX, 0), the fixed wave and block combine, lse = M + logf(S)): for a row at the same address lse_r has the bits
 *        ff_token_logprob stores.
 *   S2.  For every query q of row r, t = tok[q]:  lp = NaN if t is outside [0, vocab), and nothing is read;  otherwise lp = x_t - lse_r.
 *        x_t == -inf gives -inf; a row holding NaN or +inf gives NaN.  out[q] = lp when base is null, otherwise out[q] = base[r] + lp:
 *        one fp32 add, rounded once, never contracted with the subtraction.
 *   S3.  A row with an empty list is not read, and nothing is written for it.
 *   S4.  row_first is read as given and every bound is clamped into [0, n_q]: nothing outside tok[0 .. n_q) and out[0 .. n_q) is touched,
 *        whatever the table holds.  It is the caller's duty that the lists partition [0, n_q); then every out[q] is written exactly once.
 *   S5.  One launch, no atomics, no allocation, no host synchronisation, capturable; equal inputs give equal bits, eager or replayed.
 * FF_ERR_SHAPE: null logits, row_first, tok or out; rows <= 0, vocab <= 0, ld < vocab, n_q <= 0.  FF_ERR_UNSUPPORTED: another dtype.  Both
 * before any launch.
 * ------------------------------------------------------------------------------------------------------ */
int ff_logprob_gather(int dtype, int rows, int vocab, long long ld, const void* logits, const int* row_first, const int* tok, int n_q,
                      const float* base, float* out, ff_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * QuickGELU of the CLIP vision tower, y = x * sigmoid(1.702 x) (transformers.activations.QuickGELUActivation, selected by
 * the openai/clip-vit-* configs the reference loads in modeling_flamingo.py:70-78), and its derivative; n contiguous elements.
 * ------------------------------------------------------------------------------------------------------ */
int ff_quick_gelu_fwd(int dtype, long long n, const void* x, void* y, ff_stream_t stream);
int ff_quick_gelu_bwd(int dtype, long long n, const void* x, const void* dy, void* dx, ff_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLAMINGO_FUSION_H */
