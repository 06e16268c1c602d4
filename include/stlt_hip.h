/*
 * stlt_hip.h — C-ABI of libstlt_hip.so: the MI355X (gfx950) STLT forward hot path.
 *
 * The reference (gorjanradevski/revisiting-spatial-temporal-layouts) has no FFI: its boundary is the
 * Python class surface of src/modelling/models.py.  This header is the inner boundary the drop-in
 * `Stlt` / `StltBackbone` modules bind through ctypes; every entry point names the reference code it
 * replaces (file:line relative to the reference root).
 *
 * Conventions
 *   - extern "C"; every function returns 0 on success, a negative STLT_E* code on argument errors,
 *     or a positive hipError_t; stlt_last_error() returns a thread-local message.
 *   - all tensor arguments are raw DEVICE pointers owned by the caller (PyTorch allocations); the
 *     library never allocates or frees device memory.  It retains caller pointers in ONE place only: a training-loop context
 *     (stlt_ctx, below), which the caller creates, names in the calls that may use it, and destroys.  fp32, row-major,
 *     contiguous unless a leading dimension (ld*) is given in ELEMENTS.  ids/lengths int64, masks uint8 (1 = padded / masked).
 *   - asynchronous on `stream` (a hipStream_t passed as void*); no implicit synchronisation — the one exception
 *     is STLT_FLAG_SKIP_PADDING without the caller's row counts (stlt_inputs.n_real_tokens / n_real_frames), which reads
 *     two row counts back (one stream synchronisation per call); everything else is a fixed launch sequence that can be
 *     captured in a hipGraph.
 *   - per-thread state: the error string and the scratch lent with stlt_gemm_set_scratch (both thread-local).
 *     Process-wide: write-once caches of device properties and the routing switches (stlt_set_gemm_small_tiles,
 *     stlt_set_gemm_split_bf16, stlt_set_train_side_stream: plain integers, set them before the calls they steer, not
 *     concurrently with them).  Nothing else is process-wide: what a training loop leaves in the library between calls —
 *     the transposed weight copies of its step, its queue of deferred block weight gradients, the side stream + events of
 *     its reverse sweeps — lives in the stlt_ctx it passes to the `*_bwd` / `*_backward` calls (NULL: none of the three).
 *     A context is internally locked: calls naming the same context from several host threads are safe (reverse sweeps on
 *     the same device are serialised from their first fork to their join); different contexts never interact, so two
 *     training loops in one process — or a plain autograd backward of another model in the middle of a trainer's step —
 *     cannot read each other's copies or queue into each other's flush.
 *   - extents and alignment.  A call reads and writes only the logical extent of each operand: rows of `ld` elements are touched in
 *     their first `cols` columns only (gap columns ld - cols are neither read nor written), nothing before the base pointer or after
 *     the last logical element — two documented exceptions: stlt_gemm rounds the contraction length of contraction-major operands up
 *     to 32 rows, stlt_weight_grad_group takes rows_i in multiples of 32 (the extra rows are the caller's, zero-filled).  Scratch,
 *     workspace and tape buffers are used inside exactly the bytes their *_bytes function returns.  Every pointer has the natural
 *     alignment of its element type; each entry point below states which pointers must ALSO be 16-byte aligned (LDS-DMA of whole rows,
 *     16-byte vector loads / stores) and what it does with one that is not: "routed" = the call runs on a path of four-byte accesses,
 *     same result to rounding; "refused" = STLT_EINVAL, the message names the pointer, nothing is launched.  A row pitch that must be a
 *     multiple of 4 floats is stated with the pitch.  torch allocations are 256-byte aligned; a contiguous view such as flat[1:] is not.
 *     The whole-path, training, block, R3D and data-pipeline entry points REQUIRE 16-byte-aligned buffers throughout (parameters, inputs,
 *     outputs) and a 256-byte-aligned workspace / tape / scratch.  The forward, training and R3D calls test the latter themselves
 *     (STLT_EINVAL); a misaligned parameter or input there is the caller's error and is not promised a refusal by name.
 *     tests/test_pointer_alignment_gpu.py holds every op-level rule.
 *   - plain C: this header compiles as C99 and as C++ (tests/test_host_cpu.py builds a C client against the library).
 */
#ifndef STLT_HIP_H
#define STLT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STLT_VERSION 111  /* 111: stlt_adamw_step takes lr, beta1, beta2, eps as double (binary-incompatible: was float); 110: training-loop contexts (stlt_ctx) in the backward calls; block backward buffers split into keep / work */

#define STLT_EINVAL (-1)   /* bad shape / null pointer / unsupported size */
#define STLT_EWORKSPACE (-2) /* workspace too small */

#define STLT_ACT_NONE 0
#define STLT_ACT_GELU 1  /* exact erf GELU */
#define STLT_ACT_RELU 2  /* nn.TransformerEncoderLayer default activation (appearance branch, models.py:239-246) */

typedef void* stlt_stream_t; /* hipStream_t */

int stlt_version(void);
const char* stlt_last_error(void);

/* ---- training-loop context -------------------------------------------------------------------------------------------
 * The reference's train() (src/train.py:102-135) is one loop over one model; its state between statements lives in torch objects.
 * Here the three things a loop leaves INSIDE the library between calls hang off an explicit handle:
 *   transposed weight copies   stlt_ctx_wt_refresh .. stlt_ctx_wt_clear: current for the calls that name the context, on the device of
 *                              the refresh; every such call's stream is ordered behind the transposes by the library (an event
 *                              recorded at the end of the refresh), whatever stream the refresh ran on
 *   deferred weight gradients  stlt_ctx_dw_defer / _pending / _flush: queued by the block backwards that name the context
 *   side stream + events       of stlt_train_backward's weight-gradient products: one set per context and device, created by the first
 *                              sweep that wants it (stlt_set_train_side_stream), destroyed with the context
 * stlt_ctx_destroy: the caller has synchronised with what it enqueued through the context; queued products are dropped, copies
 * withdrawn.  Functions taking a context return STLT_EINVAL for a handle that is not live. */
typedef struct stlt_ctx stlt_ctx;
int stlt_ctx_create(stlt_ctx** out);
int stlt_ctx_destroy(stlt_ctx* ctx);

/* K1 — CategoryBoxEmbeddings.forward, src/modelling/models.py:29-39.
 * out[t,:] = LN_eps( cat_table[categories[t]] + boxes[t,0:4]·box_w^T + box_b (+ scores[t]*score_w[:,0] + score_b) )
 * scores may be NULL (key absent from the batch, models.py:33).  d % 4 == 0, d <= 2048.
 * Alignment: boxes, cat_table, box_w, box_b, score_w, score_b, ln_w, ln_b, out 16 bytes (refused otherwise); categories 8, scores 4. */
int stlt_embed_fwd(const int64_t* categories, const float* boxes, const float* scores,
                   const float* cat_table, int64_t n_categories,
                   const float* box_w, const float* box_b, const float* score_w, const float* score_b,
                   const float* ln_w, const float* ln_b, float eps,
                   int64_t n_tokens, int64_t d, float* out, stlt_stream_t stream);

/* K2/K4/K5/K6/K8 — nn.Linear (F.linear inside F.multi_head_attention_forward, linear1/linear2 of
 * nn.TransformerEncoderLayer as configured at models.py:46-52,118-124; fc1/fc2 models.py:158-163).
 * y[m, n] = act( sum_k x[m*ldx + k] * w[n*K + k] + bias[n] ),  w is (N,K) row-major (torch (out,in)).
 * M, N arbitrary.  K % 32 == 0 (every hidden size the released checkpoints use): f32-input MFMA (v_mfma_f32_32x32x2_f32), fp32
 * accumulate.  Any other K (hidden sizes like 100 or 200, which configs.py:92-111 allows): the same product and epilogues on
 * csrc/gemm_any.hip (zero-filled tiles staged through LDS by ordinary loads) — a compatibility path with the same tolerances, not a
 * tuned one.  On every route (whole tiles, small tiles, stream-K, the split-k pair for a few rows, the compatibility path, the
 * opt-in split-bf16 build) the sum over k starts from zero and the bias is added once to the finished sum, ahead of the activation:
 * an output that is mostly bias keeps fp32 error at its own scale (tests/test_product_scale_gpu.py, profiles/product_scale.md).
 * Alignment: none beyond 4 bytes.  x or w off a 16-byte boundary, or ldx % 4 != 0, is routed to that compatibility path (four-byte
 * loads); y off a 16-byte boundary or ldy % 4 != 0 takes guarded scalar stores; bias is read one float at a time.  Gap columns
 * K .. ldx-1 of x are not read, N .. ldy-1 of y not written. */
int stlt_linear_fwd(const float* x, int64_t ldx, const float* w, const float* bias,
                    float* y, int64_t ldy, int64_t M, int64_t N, int64_t K, int act, stlt_stream_t stream);

/* General product on the same kernel, used by the backward pass of nn.Linear (autograd of F.linear in the reference):
 *   c (M,N) = opA(a)·opB(b) [+ r]   with contraction length K (a multiple of 32 for the tuned kernel; any other K runs on the
 *                                   fallback of csrc/gemm_any.hip, n_split = 1 only)
 *   transA=0: a is (M,K) row-major, lda;  transA=1: a is (K,M) row-major, lda   (dW = dY^T·X)
 *   transB=0: b is (N,K) row-major, ldb;  transB=1: b is (K,N) row-major, ldb   (dX = dY·W)
 * r (nullable, ldr) is added in the epilogue (residual gradient).  n_split > 1 splits the contraction: split s writes
 * its partial product to c + s*slab_stride; sum them with stlt_reduce_slabs (deterministic, no atomics).
 * Rows of a contraction-major operand beyond the logical K must be zero-filled by the caller (K is rounded up).
 * Alignment, n_split == 1: none beyond 4 bytes — a or b off a 16-byte boundary (or lda / ldb no multiple of 4) is routed to the
 * compatibility path, r / c off it (or ldr / ldc no multiple of 4) take guarded scalar accesses.  n_split > 1 exists on the LDS-DMA
 * kernel only: a and b 16 bytes, lda % 4 == ldb % 4 == 0 (refused otherwise); c and slab_stride anywhere on 4 bytes. */
int stlt_gemm(int transA, int transB, const float* a, int64_t lda, const float* b, int64_t ldb,
              const float* r, int64_t ldr, float* c, int64_t ldc, int64_t slab_stride,
              int64_t M, int64_t N, int64_t K, int n_split, stlt_stream_t stream);
/* The same nn.Linear forward (plus an optional add-source r: y = act(x·Wᵀ + b) + r, r only with STLT_ACT_NONE) on the small-tile
 * kernel (csrc/gemm16.hip): whole tiles, no stream-K, no fix-up launch.  The `tile` parameter is columns | rows << 16 with rows 0 = 128:
 * 128 rows x {48, 64, 96, 128, 144, 192} columns, 64 rows x {64, 96, 128, 160, 192, 256}, 32 rows x {128, 192, 256}.  stlt_linear_fwd and every whole-path / training / block entry point route a product here by themselves when its launch
 * would be under-filled on the 256 x 128 tiles and the small tiles are estimated faster (few rows: the temporal tower at the
 * reference's default batch of 64 clips, the fusion models' 2048 / 2112-row blocks); stlt_linear_small_choice returns the tile
 * (same encoding) that dispatch picks for (M, N, K) — 0: the product stays on the large tiles; STLT_GEMM16=0 in the environment disables the routing.
 * This entry point runs the kernel on any shape it can take (K % 32 == 0, K >= 64, N % 4 == 0, pitches % 4 == 0) with the tile
 * given (tests, A/B measurements); other shapes return STLT_EINVAL.  Same result as stlt_linear_fwd to fp32 rounding.
 * Alignment: x, w, bias, r, y 16 bytes (refused otherwise: this entry point names the kernel).  The routing inside stlt_linear_fwd and
 * the other callers leaves a product with such a pointer, or with ldy / ldr no multiple of 4, to the large-tile / compatibility kernels. */
int stlt_linear_small_fwd(const float* x, int64_t ldx, const float* w, const float* bias, const float* r, int64_t ldr, float* y, int64_t ldy,
                          int64_t M, int64_t N, int64_t K, int act, int tile, stlt_stream_t stream);
int stlt_linear_small_choice(int64_t M, int64_t N, int64_t K);
/* The input gradient of that Linear on the same kernel: dx (M, k_in; ld_dx) = dy (M, n_out; ld_dy) · w (n_out, k_in) (+ r), the weight
 * read as it lies (no transposed copy: the [k][n] image is gathered inside the kernel).  The training sweeps (stlt_train_backward,
 * the block backwards, stlt_linear_bwd) route their under-filled dX products here by the same launch-time estimate.  tile != 0 runs it
 * on that tile (columns | rows << 16), always reading w as it lies; tile == 0 routes by the estimate — STLT_EINVAL when the estimate
 * leaves the product to the large tiles (stlt_input_grad_small_choice tells beforehand) — and, when `ctx` holds a current transposed
 * copy of w (stlt_ctx_wt_refresh), runs the product as a forward product on the copy.  n_out % 32 == 0, n_out >= 64, k_in % 4 == 0.
 * Same result as stlt_gemm(0, 1, ...) to rounding.  ctx may be NULL.
 * Alignment: dy, w, r, dx 16 bytes; ld_dx, ldr multiples of 4 (tile != 0: refused otherwise; tile == 0: such a product is not this
 * kernel's and the call returns STLT_EINVAL like any other product the estimate leaves to the large tiles). */
int stlt_input_grad_small(const float* dy, int64_t ld_dy, const float* w, int64_t n_out, int64_t k_in, const float* r, int64_t ldr, float* dx,
                          int64_t ld_dx, int64_t M, int tile, stlt_ctx* ctx, stlt_stream_t stream);
int stlt_input_grad_small_choice(int64_t M, int64_t n_out, int64_t k_in);  /* the tile the routing picks for that input gradient, reading w as it lies: columns | rows << 16 (0: large tiles) */
/* Process-wide routing switch: -1 = by the launch-time estimate (default; STLT_GEMM16 in the environment is the initial value),
 * 0 = every product on the large tiles, 1 = every product the small-tile kernel can take on it (A/B measurements), 128 / 64 / 32 = by
 * the estimate over tiles of that height only (tests, A/B; STLT_GEMM16_ROWS is the environment's form), -2 = back to the initial value
 * (what a test or tool that switched it should leave behind). */
int stlt_set_gemm_small_tiles(int mode);

/* Optional scratch for the calling thread's stlt_linear_fwd / stlt_gemm launches (torch's nn.Linear has no
 * counterpart: this is launch policy).  With scratch lent, a launch whose 256x128 output tiles would leave compute
 * units idle (fewer tiles than CUs, or a ragged last round) is cut into equal contiguous k-step ranges instead
 * ("stream-K"); tiles computed by more than one workgroup are summed in workgroup order by a second kernel, so results
 * stay deterministic.  The buffer must hold stlt_gemm_scratch_bytes() and may only be reused by work ordered after
 * the launch on its stream.  Pass NULL to withdraw.  The whole-path entry points lend a slice of their workspace.
 * The buffer is 16-byte aligned (refused otherwise); partial tiles stay inside its first stlt_gemm_scratch_bytes() bytes. */
size_t stlt_gemm_scratch_bytes(void);
int stlt_gemm_set_scratch(void* scratch, size_t bytes);
/* Weight gradients of several nn.Linear modules in ONE launch (what autograd computes product by product for
 * `loss.backward()`, src/train.py:125-127): g_w_i (n_out_i, k_in_i) += dy_i[:rows_i]^T · x_i[:rows_i] for every item.
 * dy_i (rows_i, n_out_i) and x_i (rows_i, k_in_i) row-major; rows_i a multiple of 32 (rows beyond the logical count
 * must be zero in dy or x); n_out_i, k_in_i multiples of 4; 1..32 items; items with g_w == NULL are skipped.  Needs lent
 * stream-K scratch (stlt_gemm_set_scratch).  One persistent stream-K launch over the concatenated k-step space of the
 * items + one fix-up: deterministic (fixed summation order).
 * Alignment: every dy_i and x_i 16 bytes (refused otherwise, the message names the item); g_w_i anywhere on 4 bytes (a g_w off a
 * 16-byte boundary takes guarded scalar accesses). */
typedef struct { const float* dy; int64_t n_out; const float* x; int64_t k_in; int64_t rows; float* g_w; } stlt_wgrad_item;
int stlt_weight_grad_group(const stlt_wgrad_item* items, int n_items, stlt_stream_t stream);
/* dst[i] = (accumulate ? dst[i] : 0) + sum_s slabs[s*stride + i], i < n.  Alignment: none beyond 4 bytes — slabs / dst off a 16-byte boundary
 * or a stride that is no multiple of 4 floats are routed to the element-wise kernel (another, equally fixed, summation order; n below 2^35 there, STLT_EINVAL above). */
int stlt_reduce_slabs(const float* slabs, int64_t stride, int n_slabs, float* dst, int64_t n, int accumulate,
                      stlt_stream_t stream);

/* K3 — attention core of F.multi_head_attention_forward as reached from models.py:68-71 (spatial,
 * key-padding mask) and models.py:146-150 (temporal, causal mask of utils/model_utils.py:4-7 + key padding).
 * qkv: (S*L, 3*H*dh) packed rows [q;k;v]; ctx: (S*L, H*dh).  kpm: (S*L) bytes, 1 = key masked.
 * ctx[s,i,h,:] = softmax_j( q_i·k_j/sqrt(dh) + M_ij ) v_j with M_ij = -inf if kpm[s,j] or (causal and j>i).
 * Rows whose keys are all masked produce zeros.  1 <= dh <= 256: dh == 64 (every released checkpoint) runs on the MFMA kernels; any
 * other head dim the reference's configs.py:92-111 allows runs on the vector-ALU kernels of csrc/attn_any.hip (at most 1024 keys per
 * sequence in the forward, 256 tokens a side in the backward) — the same arithmetic, masks, dropout indices and tolerances.
 * Alignment: dh == 64: qkv and ctx 16 bytes (refused otherwise: K / V rows are staged by LDS-DMA); any other dh: none beyond 4 bytes
 * (csrc/attn_any.hip falls back to four-byte accesses).  kpm: bytes. */
int stlt_attn_core_fwd(const float* qkv, const uint8_t* kpm, int causal,
                       int64_t S, int64_t L, int64_t H, int64_t dh, float* ctx, stlt_stream_t stream);

/* Fused multi-head self-attention (the north star's "fused MHSA"): the in-projection of nn.MultiheadAttention
 * (models.py:46-52,118-124: in_proj_weight (3d,d) rows [q;k;v], in_proj_bias) and the attention core in ONE kernel:
 * x (S*L, d) -> ctx (S*L, d), the packed QKV tensor never goes to memory.  stlt_mhsa_fused_fwd is the temporal tower's form
 * (causal mask of utils/model_utils.py:4-7 + src_key_padding_mask_frames, models.py:142-150).  Sequences of 1 <= L <= 64 tokens
 * (the reference's layouts are T = layout_num_frames + 1 = 17 / 33, datasets.py:97-113; Action Genome 64) and 64-channel heads
 * (d == 64*H); other shapes return STLT_EINVAL (callers use stlt_linear_fwd + stlt_attn_core_fwd).  Same result as that pair to
 * fp32 rounding.
 * Alignment (both forms): x, in_proj_w, ctx and qkv_out 16 bytes (refused otherwise); in_proj_b 4 bytes; kpm bytes. */
int stlt_mhsa_fused_fwd(const float* x, const float* in_proj_w, const float* in_proj_b, const uint8_t* kpm, int64_t S, int64_t L,
                        int64_t H, int64_t d, float* ctx, stlt_stream_t stream);
/* The same kernel with every option: causal = 0 is the spatial tower's form (key-padding mask only, models.py:68-71; L up to
 * ~36 tokens); qkv_out != NULL also writes the packed projections (S*L, 3d) — what a training forward keeps for the reverse
 * sweep; dropout_p > 0 (needs qkv_out) drops attention probabilities with the library's counter mask at `site`, element index
 * ((query token * H + head) << 8) | key position, exactly as stlt_attn_core_fwd_train does, so stlt_attn_core_bwd regenerates it. */
int stlt_mhsa_fused_fwd_ex(const float* x, const float* in_proj_w, const float* in_proj_b, const uint8_t* kpm, int causal, int64_t S,
                           int64_t L, int64_t H, int64_t d, float dropout_p, uint64_t seed, uint32_t site, float* ctx, float* qkv_out,
                           stlt_stream_t stream);
/* 1 when stlt_forward / stlt_backbone_forward / stlt_train_forward run their temporal layers through the fused kernel for this
 * shape at 1024 clips per launch (64-channel heads, T <= 64 frames; the launch-time estimate of csrc/mhsa.hip compares the fused
 * launch with the in-projection + attention-core pair: T = 17, 32, 64 take the fused kernel, T = 33 — 99 of a work item's 128 rows —
 * keeps the pair; STLT_FUSED_MHSA=0 in the environment switches the fused kernel off).  stlt_fused_mhsa_used answers for one
 * launch of S sequences of L tokens (causal: temporal tower, else the spatial tower): small launches (64 clips) go to the pair,
 * whose in-projection then runs on the small-tile kernel. */
int stlt_fused_mhsa_active(int64_t T, int64_t d, int64_t H);
int stlt_fused_mhsa_used(int64_t S, int64_t L, int64_t d, int64_t H, int causal);
/* Cross-attention core (CrossAttentionLayer of CAF/CACNF, models.py:362-382; also self-attention on unpacked buffers):
 * queries q (S*Lq rows, stride ldq floats) attend to keys k / values v (S*Lk rows, stride ldkv).  kpm: (S*Lk) bytes over
 * the KEY tokens (pass zeros for no padding mask).  ctx: (S*Lq, H*dh).  causal requires Lq == Lk.
 * ldq, ldkv multiples of 4; columns H*dh .. ld-1 of a row are not read.  Alignment: dh == 64: q, k, v, ctx 16 bytes (refused
 * otherwise); any other dh: none beyond 4 bytes. */
int stlt_attn_cross_fwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const uint8_t* kpm,
                        int causal, int64_t S, int64_t Lq, int64_t Lk, int64_t H, int64_t dh, float* ctx,
                        stlt_stream_t stream);

/* K3 on a ragged layout: self-attention over M compacted rows of a packed (M, 3*H*dh) buffer cut into variable-length
 * segments (one frame's objects, one clip's frames) — what STLT_FLAG_SKIP_PADDING runs instead of the padded K3.
 * seg_start[r] / seg_end[r] (int32, device): first row / one past the last row of row r's segment; segments are
 * contiguous and cover [0, M).  ctx[r] = softmax over the keys of r's segment (only those at rows <= r when causal).
 * Alignment: dh == 64: qkv and ctx 16 bytes (refused otherwise); any other dh: none beyond 4 bytes.  seg_start / seg_end: 4 bytes. */
int stlt_attn_ragged_fwd(const float* qkv, const int32_t* seg_start, const int32_t* seg_end, int causal, int64_t M,
                         int64_t H, int64_t dh, float* ctx, stlt_stream_t stream);

/* Residual + LayerNorm (norm1/norm2 of nn.TransformerEncoderLayer, eps 1e-5; ClassificationHead.layer_norm
 * models.py:159,163 with res == NULL).  out[m,:] = LN_eps( x[m*ldx + :] + res[m*ldres + :] ).
 * d % 4 == 0, d <= 2048; ldx, ldres, ldout multiples of 4, columns d .. ld-1 neither read nor written.  Alignment: x, res, ln_w, ln_b,
 * out 16 bytes (refused otherwise). */
int stlt_add_layernorm_fwd(const float* x, int64_t ldx, const float* res, int64_t ldres,
                           const float* ln_w, const float* ln_b, float eps,
                           int64_t M, int64_t d, float* out, int64_t ldout, stlt_stream_t stream);

/* K7 — CLS select (models.py:79) + FramesEmbeddings.forward (models.py:98-111).
 * out[b,t,:] = LN_eps( spatial[(b*T+t)*row_stride + :] + pos_table[t] + type_table[frame_types[b,t]] ).
 * row_stride % 4 == 0; only the first d floats of a row are read.  Alignment: spatial, pos_table, type_table, ln_w, ln_b, out 16 bytes
 * (refused otherwise); frame_types 8. */
int stlt_frames_embed_fwd(const float* spatial, int64_t row_stride, const int64_t* frame_types,
                          const float* pos_table, const float* type_table,
                          const float* ln_w, const float* ln_b, float eps,
                          int64_t B, int64_t T, int64_t d, float* out, stlt_stream_t stream);

/* K8a — Stlt.forward gather, models.py:189-192: out[b,:] = x[b, lengths[b]-1, :] for batch-major x (B,T,d).
 * Alignment: x and out 16 bytes (refused otherwise); lengths 8. */
int stlt_gather_last_fwd(const float* x, const int64_t* lengths, int64_t B, int64_t T, int64_t d,
                         float* out, stlt_stream_t stream);

/* Collater on the device — padding + mask half of StltCollater.__call__, src/modelling/datasets.py:243-288 (pad_sequence:
 * src/utils/data_utils.py:93-102).  Inputs are the per-video tensors of StltDataset.__getitem__ (datasets.py:52-125)
 * concatenated along the frame axis: video b owns frames [frame_offsets[b], frame_offsets[b+1]); outputs are the padded
 * (B,T,N,.) batch and both key-padding masks (uint8, 1 = padded).  Frames past a video's length carry the CLS object in
 * slot 0 (category cls_id, box [0,0,1,1], score 1) and frame type 0.  scores_ragged/scores are NULL together
 * (datasets.py:253-260 keeps scores only for action_genome).
 * Alignment: boxes_ragged and boxes 16 bytes (refused otherwise: a box is one 16-byte access); the int64 arrays 8, scores 4, masks bytes. */
int stlt_collate_fwd(const int64_t* categories_ragged, const float* boxes_ragged, const float* scores_ragged,
                     const int64_t* frame_types_ragged, const int64_t* frame_offsets, int64_t B, int64_t T, int64_t N,
                     int64_t cls_id, int64_t* categories, float* boxes, float* scores, int64_t* frame_types,
                     uint8_t* kpm_boxes, uint8_t* kpm_frames, stlt_stream_t stream);

/* Device video collater (csrc/video.hip) — the per-frame transforms of AppearanceDataset.__getitem__ (src/modelling/datasets.py:163-208):
 * Resize(floor(1.15 S)) with Pillow's 8-bit antialiased bilinear resampling, VideoColorJitter in training (src/utils/data_utils.py:110-137),
 * the crop, ToTensor + Normalize, written as video_frames (B, 3, T, S, S) float32 — the reference's values bit for bit.
 * One descriptor per clip; its T frames lie in `frames` (device memory) at src_offset as (T, h, w, 3) uint8.  A resample table for an
 * axis of size in -> out holds `out` (first, count) pairs of int32 followed by out x ksize int32 weights (22 fraction bits); an axis
 * whose size stays has no table (offset -1), as Pillow runs no pass there.  `clips`, `tables` (n_table int32) and `lut` (256 float32:
 * the normalised value of each uint8) are HOST memory: every descriptor and table entry is checked against the frame sizes, the crop,
 * the packed buffer and the table buffer before anything is copied or launched (STLT_EINVAL otherwise), then they are copied into the
 * workspace on `stream`; pinned host memory must stay untouched until the stream has passed the call. */
typedef struct {
  int64_t src_offset;      /* byte offset of the clip's first frame in `frames` */
  int32_t h, w;            /* source frame size */
  int32_t rh, rw;          /* resized frame size */
  int32_t top, left;       /* crop origin in the resized frame; the S x S crop lies inside it */
  int32_t tab_x, ksize_x;  /* horizontal table: offset in `tables` and taps per output column; -1 when rw == w */
  int32_t tab_y, ksize_y;  /* vertical table: likewise; -1 when rh == h */
  int32_t jitter;          /* 0: evaluation; 1: colour jitter, the four ops in order[] */
  int32_t order[4];        /* a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue */
  float brightness, contrast, saturation;
  int32_t hue_shift;       /* np.uint8(hue_factor * 255), 0..255 */
} stlt_video_clip;
size_t stlt_video_prep_workspace_bytes(int64_t B, int64_t T, int64_t n_table); /* 0 for a bad shape */
int stlt_video_prep_fwd(const uint8_t* frames, int64_t frames_bytes, const stlt_video_clip* clips, const int32_t* tables, int64_t n_table,
                        const float* lut, int64_t B, int64_t T, int64_t S, float* out, void* workspace, size_t workspace_bytes,
                        stlt_stream_t stream);

/* Device layout dataset (csrc/layout_data.hip, layout_data.py) — StltDataset.__getitem__ (src/modelling/datasets.py:52-125) and
 * StltCollater (datasets.py:239-288) over annotation tables uploaded once.
 * stlt_layout_boxes_fwd: fix_box (src/utils/data_utils.py:205-231) and `torch.tensor(box) / video_size` (datasets.py:75-80) for
 * n_objects kept objects.  raw_boxes (n, 4) int32 hold max(0, int(b)) saturated at 2^30, sizes (n, 2) int32 the (w, h) of each
 * object's video (1 <= w, h <= 2^24, not checked: device memory); boxes (n, 4) float32.  raw_boxes / boxes 16-byte aligned.
 * stlt_layout_batch_fwd: one batch, written the way StltCollater pads it.  batch_host is HOST memory of B * (2 + T) int32: the
 * video index of each clip, its number of sampled frames (<= T), then B rows of T frame indices (the first count[b] used).  Every
 * index and every offset it leads to (video_frames_host, frame_objects_host, the action lists) is checked on the host (STLT_EINVAL)
 * before it is copied to batch_dev (device, same size) on `stream` and the kernel is launched; pinned host memory must stay
 * untouched until the stream has passed the call.  Outputs (L >= 1 + the largest count): categories (B, L, N) int64, boxes
 * (B, L, N, 4) float32 (16-byte aligned), scores (B, L, N) float32 or NULL, frame_types (B, L) int64, kpm_boxes (B, L, N) and
 * kpm_frames (B, L) uint8 (1 = padded), lengths (B) int64 = count + 1, labels: (B) int64 video_label when n_classes == 0, else
 * (B, n_classes) float32 multi-hot of the video's actions.  Sampled frames carry CLS (cls_id, [0,0,1,1], score 1), their kept
 * objects, then zero slots, and type empty / regular by frame_empty; frame count[b] is the extract frame; later frames are padding
 * (CLS alone, type 0).  No synchronisation, no allocation: the call can be captured. */
typedef struct {
  int64_t n_videos, n_frames, n_objects, n_actions;
  int64_t n_classes;                               /* 0: single-label (video_label); > 0: multi-hot width */
  int64_t cls_id, type_regular, type_empty, type_extract;  /* category2id["cls"], frame2type (configs.py:25-90); "pad" is 0 */
  const int64_t* video_frames_host;   /* HOST (n_videos + 1): video v owns frames [video_frames[v], video_frames[v + 1]) */
  const int64_t* frame_objects_host;  /* HOST (n_frames + 1): frame f owns kept objects [frame_objects[f], frame_objects[f + 1]) */
  const int64_t* video_actions_host;  /* HOST (n_videos + 1), multi-hot only: video v owns actions [video_actions[v], ...[v + 1]) */
  const int32_t* actions_host;        /* HOST (n_actions), multi-hot only: class indices */
  const int64_t* video_frames;        /* device copies of the four above, then the device-only tables */
  const int64_t* frame_objects;
  const uint8_t* frame_empty;         /* (n_frames): frame_objects was empty before thresholding */
  const int32_t* object_category;     /* (n_objects) */
  const float* object_score;          /* (n_objects) */
  const float* object_box;            /* (n_objects, 4): stlt_layout_boxes_fwd's output */
  const int64_t* video_label;         /* (n_videos), single-label only */
  const int64_t* video_actions;
  const int32_t* actions;
} stlt_layout_table;
int stlt_layout_boxes_fwd(const int32_t* raw_boxes, const int32_t* sizes, int64_t n_objects, float* boxes, stlt_stream_t stream);
int stlt_layout_batch_fwd(const stlt_layout_table* table, const int32_t* batch_host, int32_t* batch_dev, int64_t B, int64_t T, int64_t L,
                          int64_t N, int64_t* categories, float* boxes, float* scores, int64_t* frame_types, uint8_t* kpm_boxes,
                          uint8_t* kpm_frames, int64_t* lengths, void* labels, stlt_stream_t stream);

/* Device frame store (csrc/frame_store.hip, frame_data.py) — AppearanceDataset.__getitem__ (src/modelling/datasets.py:163-208) split at
 * the step that does not depend on the batch: the reference resizes every frame on its own before any random transform
 * (datasets.py:172-177), and Pillow's result is an 8-bit image, so the resized frame is computed once and kept on the device as uint8.
 * stlt_frames_resize_fwd: the Resize of datasets.py:147,173 for n frames (n, h, w, 3) uint8 in device memory `src`: Pillow's antialiased
 * bilinear filter as two 8-bit passes, horizontal then vertical, each only on an axis whose size changes; (n, rh, rw, 3) uint8 is
 * written at store + dst_offset.  tab_x / tab_y are HOST tables in stlt_video_clip's layout (`out` (first, count) pairs, then
 * out x ksize int32 weights), NULL for an axis that keeps its size; every entry is checked against the source axis (STLT_EINVAL)
 * before they are copied into the workspace and anything is launched.  Workspace: stlt_frames_resize_workspace_bytes (0 for a bad shape).
 * stlt_frames_batch_fwd: VideoColorJitter in training (src/utils/data_utils.py:110-137), the crop (datasets.py:181-194), ToTensor +
 * Normalize (datasets.py:149-152) and AppearanceCollater's stack (datasets.py:291-300): video_frames (B, 3, T, S, S) float32 (16-byte
 * aligned), the reference's values bit for bit, from resized frames.  batch_host is HOST memory of stlt_frames_batch_block_bytes(B, T):
 * B x T int64 byte offsets, one per sampled frame (frames of a clip need not be contiguous or distinct), then B descriptors.  An
 * offset below store_bytes addresses `store`, one in [store_bytes, store_bytes + spill_bytes) the spill area `spill` (frames of
 * videos that are not resident, resized for this batch); both are device memory, start on a 4-byte boundary and have sizes that
 * are multiples of 4, because rows are read as whole aligned dwords (either may be NULL with size 0).  Every descriptor, crop and
 * offset is checked on the host against the frame and buffer sizes (STLT_EINVAL) before the block is copied to batch_dev (device, same
 * size, 8-byte aligned) on `stream` and the kernels are launched; pinned host memory must stay untouched until the stream has passed
 * the call.  lut: 256 float32 in DEVICE memory, the normalised value of each uint8.  sums: B x T uint64 of device scratch, needed
 * when any clip has jitter = 1 (the contrast step's grey mean of the whole frame).  S <= 1024.  No synchronisation, no allocation:
 * the call can be captured. */
typedef struct {
  int32_t rh, rw;          /* resized frame size: every frame of the clip holds rh x rw x 3 bytes */
  int32_t top, left;       /* crop origin in the resized frame; the S x S crop lies inside it */
  int32_t jitter;          /* 0: evaluation; 1: colour jitter, the four ops in order[] */
  int32_t order[4];        /* a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue */
  float brightness, contrast, saturation;
  int32_t hue_shift;       /* np.uint8(hue_factor * 255), 0..255 */
  int32_t reserved;        /* keeps the descriptor a multiple of 8 bytes */
} stlt_frames_clip;
size_t stlt_frames_resize_workspace_bytes(int64_t n, int64_t h, int64_t w, int64_t rh, int64_t rw, int64_t ksize_x, int64_t ksize_y);
int stlt_frames_resize_fwd(const uint8_t* src, int64_t n, int64_t h, int64_t w, int64_t rh, int64_t rw, const int32_t* tab_x, int64_t ksize_x,
                           const int32_t* tab_y, int64_t ksize_y, uint8_t* store, int64_t store_bytes, int64_t dst_offset, void* workspace,
                           size_t workspace_bytes, stlt_stream_t stream);
size_t stlt_frames_batch_block_bytes(int64_t B, int64_t T); /* 0 for a bad shape */
int stlt_frames_batch_fwd(const uint8_t* store, int64_t store_bytes, const uint8_t* spill, int64_t spill_bytes, const void* batch_host,
                          void* batch_dev, const float* lut, int64_t B, int64_t T, int64_t S, uint64_t* sums, float* out, stlt_stream_t stream);

/* ---- whole-path entry points (host-side orchestration in native code) ---- */

typedef struct {
  const float *in_proj_w, *in_proj_b;   /* (3d,d) rows [q;k;v], (3d) */
  const float *out_proj_w, *out_proj_b; /* (d,d), (d) */
  const float *lin1_w, *lin1_b;         /* (4d,d), (4d) */
  const float *lin2_w, *lin2_b;         /* (d,4d), (d) */
  const float *norm1_w, *norm1_b, *norm2_w, *norm2_b; /* (d) each, eps 1e-5 */
} stlt_layer_params;

typedef struct {
  int64_t d, H, n_categories, n_spatial, n_temporal, n_classes, n_positions;
  float ln_eps; /* config.layer_norm_eps (1e-12) — the three explicit LayerNorms only */
  const float *cat_emb, *box_w, *box_b, *score_w, *score_b, *emb_ln_w, *emb_ln_b; /* models.py:19-27 */
  const float *pos_emb, *type_emb, *frames_ln_w, *frames_ln_b;                    /* models.py:88-93 */
  const stlt_layer_params* spatial;  /* HOST array [n_spatial]  (models.py:53-55) */
  const stlt_layer_params* temporal; /* HOST array [n_temporal] (models.py:126-128) */
  const float *fc1_w, *fc1_b, *head_ln_w, *head_ln_b, *fc2_w, *fc2_b; /* models.py:158-160; may be NULL for backbone-only */
} stlt_params;

typedef struct {
  int64_t B, T, N;
  const int64_t* categories;   /* (B,T,N) */
  const float* boxes;          /* (B,T,N,4) */
  const float* scores;         /* (B,T,N) or NULL */
  const uint8_t* kpm_boxes;    /* (B,T,N)  src_key_padding_mask_boxes */
  const int64_t* frame_types;  /* (B,T) */
  const uint8_t* kpm_frames;   /* (B,T)    src_key_padding_mask_frames */
  const int64_t* lengths;      /* (B) */
  /* STLT_FLAG_SKIP_PADDING only, optional (0 = unknown): the batch's real rows as the collater can count them on the host —
   * n_real_frames = number of zeros in kpm_frames, n_real_tokens = number of zeros in kpm_boxes inside those frames.  With both given the
   * call reads nothing back: no stream synchronisation, capturable in a hipGraph.  In the inference calls (stlt_forward, stlt_backbone_forward,
   * stlt_caf_forward_flags) the two numbers may be UPPER BOUNDS: the rows between the real counts and the bounds are computed as
   * self-contained dummy rows nobody reads, so one captured graph serves every batch whose counts stay below the bounds it was captured
   * with (a bucket, a percentile of the dataset).  The training calls need the exact counts (a dummy row would leave a gradient).  Either way
   * they are verified on the device: real counts above the bounds (training: different from them), or masks that break the collater contract,
   * give NaN results instead of an error return. */
  int64_t n_real_tokens, n_real_frames;
} stlt_inputs;

#define STLT_FLAG_CLS_ONLY_LAST_SPATIAL 1 /* last spatial layer: Q/out-proj/FFN on the CLS rows only (the only rows read, models.py:79) */
#define STLT_FLAG_SKIP_PADDING 4 /* stlt_forward with out_btd == NULL: compute the real (unmasked) tokens and frames only.  Same logits: a padded row is
                                   masked as a key everywhere and never read as a query result.  Implies both flags above.  Needs collater-shaped
                                   masks (slot 0 of a real frame unmasked, frame lengths-1 real); synchronises the stream once per call unless stlt_inputs carries
                                   the batch's two row counts (n_real_tokens / n_real_frames). */
#define STLT_FLAG_TRAIN_UPPER_ONLY 8   /* stlt_train_backward: stop after the prediction head and the temporal tower (their gradients are final) */
#define STLT_FLAG_TRAIN_LOWER_ONLY 16  /* stlt_train_backward: resume from there (frames embeddings, spatial tower, token embeddings); the scratch must be
                                          untouched in between.  Lets a data-parallel caller all-reduce the upper gradients while the lower half runs. */
#define STLT_FLAG_TRAIN_BACKBONE 32     /* stlt_train_forward / _backward as the StltBackbone of a fusion model (models.py:136-152 inside :446-483): no
                                         * prediction head, every temporal layer on every frame; the forward's `logits` argument receives the (B*T, d)
                                         * backbone output and the backward's `dlogits` argument is its gradient (B*T, d).  Not with STLT_FLAG_SKIP_PADDING. */
#define STLT_FLAG_LAST_ROW_ONLY_TEMPORAL 2 /* stlt_forward with out_btd == NULL: last temporal layer's out-proj/FFN on the rows at lengths-1 only (models.py:189-192) */

/* bytes of scratch the whole-path calls need for this shape */
size_t stlt_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_classes);

/* StltBackbone.forward, models.py:136-152.  out_btd is batch-major (B,T,d); the module returns its (T,B,d) view. */
int stlt_backbone_forward(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes,
                          int flags, float* out_btd, stlt_stream_t stream);

/* Stlt.forward, models.py:185-195: backbone -> gather at lengths-1 -> ClassificationHead.  logits (B,n_classes).
 * out_btd may be NULL (then the backbone output lives in the workspace). */
int stlt_forward(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes,
                 int flags, float* out_btd, float* logits, stlt_stream_t stream);

/* ---- Per-prefix logits: Stlt's prediction after every number of observed frames, in one pass ----
 * The temporal tower is causal (models.py:136-152) and the clip is read out at the extract frame the dataset appends behind the sampled
 * frames (datasets.py:97-113, models.py:185-195), so "the logits after t observed frames" are Stlt.forward on frames 0 .. t-1 of the clip
 * followed by the clip's own extract frame (the frame at lengths-1), lengths = t+1.  Spatial tower and frame rows of the temporal tower
 * are shared by all prefixes of a clip; only the extract token differs.  It runs as a second stream of B*T "probe" rows: probe (b,t) is
 * the clip's extract frame embedded at position t, which in every temporal layer attends to the frame stream's keys j < t and to itself. */

/* Probe attention of one temporal layer (extends the attention of models.py:136-152 to the probe stream).  qkv_frames, qkv_probes:
 * (S*T, 3*H*dh) packed rows [q;k;v] of the frame stream and of the probe stream (same in-projection); kpm: (S*T) bytes, 1 = frame masked
 * as a key; ctx: (S*T, H*dh).  ctx[s,t,h,:] = softmax over { q_p[s,t]·k_f[s,j]/sqrt(dh) : j < t, kpm[s,j] == 0 } and q_p[s,t]·k_p[s,t]/sqrt(dh)
 * of { v_f[s,j] }, v_p[s,t].  The own key is always present: no row is fully masked, ctx[s,0] = v_p[s,0].  Probes never see other probes;
 * the queries of qkv_frames are not read.  Any T >= 1 (key tiles with an online softmax), 1 <= dh <= 256.
 * Alignment: qkv_frames, qkv_probes, ctx 16 bytes (refused otherwise); kpm bytes. */
int stlt_attn_prefix_probe_fwd(const float* qkv_frames, const float* qkv_probes, const uint8_t* kpm, int64_t S, int64_t T, int64_t H,
                               int64_t dh, float* ctx, stlt_stream_t stream);

/* bytes of scratch stlt_forward_prefixes needs for this shape (0 for an empty shape) */
size_t stlt_prefix_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_classes);

/* Stlt.forward (models.py:185-195 on the backbone of models.py:136-152) for every prefix of every clip.  logits: (B,T,n_classes);
 * logits[b,t] for t < lengths[b] is what stlt_forward returns for the batch cut to frames 0 .. t-1 of clip b followed by its extract frame
 * (t = 0: the extract frame alone; t = lengths[b]-1: stlt_forward's own logits); entries t >= lengths[b] are written as 0.
 * Inference only, padded schedule.  flags: STLT_FLAG_CLS_ONLY_LAST_SPATIAL is honoured, STLT_FLAG_LAST_ROW_ONLY_TEMPORAL is ignored,
 * STLT_FLAG_SKIP_PADDING is refused (STLT_EINVAL).  In the last temporal layer the frame stream is only projected to keys and values.
 * No allocation, no synchronisation, capturable.  workspace: 256-byte aligned, stlt_prefix_workspace_bytes. */
int stlt_forward_prefixes(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes, int flags, float* logits,
                          stlt_stream_t stream);

/* ---- attention maps: what the model looked at (extends the nn.MultiheadAttention layers of models.py:46-55,118-128 by their
 * need_weights=True output, which the reference's encoder layers discard) ---- */

/* Attention probabilities of K3 (what nn.MultiheadAttention returns with need_weights=True), same arguments and masks as stlt_attn_core_fwd.
 * per_head == 0: probs (S, L, L),    probs[s,i,j]   = (1/H) * sum_h softmax_j( q_i·k_j/sqrt(dh) + M_ij )   (average_attn_weights=True)
 * per_head == 1: probs (S, H, L, L), probs[s,h,i,j] = softmax_j( ... ) of head h                           (average_attn_weights=False)
 * M_ij = -inf if kpm[s,j] or (causal and j > i).  Masked entries are written as exactly 0; a query row whose keys are all masked is
 * written as zeros (the core's rule for ctx); every element of probs is written, none is left uninitialised.  Query rows are NOT
 * filtered by kpm: a padded token's row holds what the reference computes for it.  The head average is summed head by head in
 * registers (no atomics): the same bits on every run.
 * 1 <= L <= 1024, 1 <= dh <= 256; dh == 64 with L <= 64 (every released checkpoint, every layout of the reference) runs on the MFMA
 * kernel of csrc/attn_probs.hip, everything else on its vector-ALU kernel.
 * Alignment: dh == 64: qkv 16 bytes (refused otherwise); other dh: 4 bytes; probs 4 bytes; kpm bytes. */
int stlt_attn_probs_fwd(const float* qkv, const uint8_t* kpm, int causal, int64_t S, int64_t L, int64_t H, int64_t dh,
                        int per_head, float* probs, stlt_stream_t stream);

/* The same for queries and keys that lie in different buffers and differ in number: stlt_attn_cross_fwd without its value half — what the
 * nn.MultiheadAttention of the fusion models' CrossAttentionLayer (models.py:362-382, called at 411-419) returns with need_weights=True.
 * q rows are ldq floats apart ((S*Lq) rows), k rows ldk floats apart ((S*Lk) rows); only the first H*dh columns of either are read.
 * per_head == 0: probs (S, Lq, Lk);  per_head == 1: probs (S, H, Lq, Lk);  probs[s,(h,)i,j] = softmax_j( q_i·k_j/sqrt(dh) + M_ij ),
 * M_ij = -inf if kpm[s*Lk + j] or (causal and j > i).  kpm: (S*Lk) bytes over the key tokens, never NULL (zeros for no mask); causal
 * requires Lq == Lk.  Masked entries are written as exactly 0, a query row whose keys are all masked as zeros, every element of probs is
 * written; query rows are not filtered by any mask.  The head average is summed head by head in registers in a fixed order (no atomics):
 * the same bits on every run.
 * 1 <= Lq, Lk <= 1024, 1 <= dh <= 256.  dh == 64 with Lk <= 64 (any Lq) runs on the MFMA kernel of csrc/attn_probs.hip and needs q
 * and k 16-byte aligned and ldq, ldk multiples of 4 (refused otherwise); everything else on its vector-ALU kernel, pointers and strides
 * 4 bytes.  probs 4 bytes; kpm bytes.  Every bad argument is STLT_EINVAL and launches nothing. */
int stlt_attn_probs_cross_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const uint8_t* kpm, int causal, int64_t S, int64_t Lq,
                              int64_t Lk, int64_t H, int64_t dh, int per_head, float* probs, stlt_stream_t stream);

/* bytes of scratch stlt_forward_attention needs for this shape (0 for an empty shape) */
size_t stlt_attention_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_classes);

/* Stlt.forward (models.py:185-195) on the dense padded schedule, also writing every layer's attention probabilities.
 * attn_spatial:  (n_spatial, B, T, N, N)  [per_head: (n_spatial, B, T, H, N, N)]  or NULL
 * attn_temporal: (n_temporal, B, T, T)    [per_head: (n_temporal, B, H, T, T)]    or NULL
 * Layer-major: each layer's launch writes one contiguous block (stlt_attn_probs_fwd on the layer's packed QKV).  With a map requested,
 * N (spatial) / T (temporal) is at most 1024.  logits (B, n_classes) as stlt_forward with flags == 0 — to fp32 rounding, not bit for bit:
 * every layer here runs the unfused pair (in-projection into a packed QKV buffer, then the attention core), never the fused MHSA kernel,
 * which has no QKV in memory; a NULL map changes neither the other outputs nor the launches that produce them.
 * Inference only.  Every layer runs on every row: the elision flags (STLT_FLAG_CLS_ONLY_LAST_SPATIAL, STLT_FLAG_LAST_ROW_ONLY_TEMPORAL)
 * are ignored, STLT_FLAG_SKIP_PADDING is refused (STLT_EINVAL).  A workspace smaller than stlt_attention_workspace_bytes is refused with
 * STLT_EINVAL as well.  Nothing is launched by a refused call.
 * No allocation, no synchronisation, capturable.  workspace: 256-byte aligned.  logits, attn_spatial, attn_temporal: 4 bytes. */
int stlt_forward_attention(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes, int flags, int per_head,
                           float* logits, float* attn_spatial, float* attn_temporal, stlt_stream_t stream);

/* ---- CAF / CACNF on precomputed appearance features (reference models.py:230-271, 286-298, 328-549) ----
 * The layout branch is the StltBackbone above; the appearance branch starts from the R3D-50 feature map the reference's
 * Resnet3D.forward_features returns, (B, 2048, 2,4,4) = (B, feat_channels, app_tokens) row-major, given by the caller. */
typedef struct {  /* SelfAttentionLayer / CrossAttentionLayer: nn.MultiheadAttention + LayerNorm(eps = ln_eps), models.py:345-382 */
  const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *ln_w, *ln_b;
} stlt_attn_block_params;
typedef struct {  /* FeedforwardModule, models.py:328-342 */
  const float *lin1_w, *lin1_b, *lin2_w, *lin2_b, *ln_w, *ln_b;
} stlt_ffn_block_params;
typedef struct {  /* CrossModalModule, models.py:385-431; cross_attn is shared by both directions, appearance_ffn IS a self-attention layer */
  stlt_attn_block_params cross_attn, layout_attn, appearance_attn, appearance_ffn;
  stlt_ffn_block_params layout_ffn;
} stlt_crossmodal_params;
typedef struct {  /* ClassificationHead (d->d->K) or FusionHead (2d->d->K): fc1, LayerNorm(ln_eps), fc2 */
  const float *fc1_w, *fc1_b, *ln_w, *ln_b, *fc2_w, *fc2_b;
} stlt_head_params;
typedef struct {
  stlt_params layout;                 /* layout_branch (head fields unused) */
  int64_t feat_channels, app_tokens;  /* 2048, 32 */
  const float *proj_w, *proj_b;       /* projector Conv3d 1x1x1 == Linear (d, feat_channels), models.py:236-238 */
  const float *cls_token, *pos_embed; /* (d), (app_tokens+1, d), models.py:247-250 */
  int64_t n_app_layers;
  const stlt_layer_params* app_layers; /* HOST array; ReLU encoder layers, LN eps 1e-5, models.py:239-246 */
  int64_t n_fusion;
  const stlt_crossmodal_params* fusion; /* HOST array */
  stlt_head_params fusion_head;        /* FusionHead: classifier (CAF) / fusion_classifier (CACNF) */
  stlt_head_params layout_head, appearance_head; /* CACNF only (ClassificationHead x2); fc1_w == NULL for CAF */
} stlt_caf_params;

size_t stlt_caf_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t feat_channels, int64_t app_tokens,
                                int64_t n_classes);
/* CrossAttentionFusion.forward (models.py:486-498) -> logits_caf (B,K).  With the two extra heads given it is
 * CrossAttentionCentralNetFusion.forward (models.py:520-549): logits_stlt, logits_resnet3d, logits_caf and
 * logits_ensemble = their mean (all (B,K); the three extra outputs may be NULL for CAF). */
int stlt_caf_forward(const stlt_caf_params* p, const stlt_inputs* in, const float* appearance_features, void* workspace,
                     size_t workspace_bytes, float* logits_caf, float* logits_stlt, float* logits_resnet3d,
                     float* logits_ensemble, stlt_stream_t stream);
/* The same with STLT_FLAG_SKIP_PADDING accepted in `flags`: the layout branch runs on the real tokens / frames only (the
 * collater's masks, as for stlt_forward); padded frames' rows of the (B,T,d) layout state are zero — downstream they are
 * only masked keys (models.py:403-431) — so the logits are those of the padded schedule to rounding.  Like stlt_forward
 * with that flag it synchronises the stream once (two row counts are read back to size the launches) unless stlt_inputs carries them. */
int stlt_caf_forward_flags(const stlt_caf_params* p, const stlt_inputs* in, const float* appearance_features, void* workspace,
                           size_t workspace_bytes, int flags, float* logits_caf, float* logits_stlt, float* logits_resnet3d,
                           float* logits_ensemble, stlt_stream_t stream);

/* ---- attention maps of the fusion models: the need_weights=True output of every nn.MultiheadAttention the forward above runs, which the
 * reference's SelfAttentionLayer / CrossAttentionLayer discard with [0] (models.py:353-388), beside the layout branch's (models.py:46-55,
 * 118-128) and the appearance encoder's (models.py:239-246).  A = app_tokens + 1 ---- */
typedef struct {            /* every pointer nullable; head-averaged shapes, per_head inserts H before the last two dims */
  float *spatial;              /* (n_spatial, B, T, N, N)   per_head: (n_spatial, B, T, H, N, N) — layout branch, as stlt_forward_attention */
  float *temporal;             /* (n_temporal, B, T, T)     — layout branch, causal + frame padding */
  float *appearance;           /* (n_app_layers, B, A, A)   — appearance encoder, no mask */
  float *layout_to_appearance; /* (n_fusion, B, T, A)       cross_attn, queries = layout frames (models.py:411-414), no mask */
  float *appearance_to_layout; /* (n_fusion, B, A, T)       cross_attn, queries = appearance tokens, keys masked by kpm_frames (415-419) */
  float *fusion_layout;        /* (n_fusion, B, T, T)       layout_attn: causal + kpm_frames (421-425) */
  float *fusion_appearance;    /* (n_fusion, 2, B, A, A)    [.,0] appearance_attn, [.,1] appearance_ffn (a SelfAttentionLayer, models.py:401) */
} stlt_caf_attention_maps;
/* bytes of scratch stlt_caf_forward_attention needs (the buffers of stlt_caf_forward: every block's Q and K already lie in them) */
size_t stlt_caf_attention_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t feat_channels, int64_t app_tokens,
                                          int64_t n_classes);
/* stlt_caf_forward (models.py:446-483, 486-498, 520-549; LCF with n_fusion == 0: models.py:296-322) also writing the attention
 * probabilities of every layer whose sink in `maps` is not NULL (maps == NULL: none).  One launch sequence serves both entry points: behind
 * each attention core one stlt_attn_probs_fwd (self-attention: the layer's packed QKV) or stlt_attn_probs_cross_fwd (the two cross blocks:
 * the projected queries, ldq = d, and the packed K/V, ldk = 2d, with the key-side mask the block uses) on the core's own buffers; a NULL
 * sink skips that launch and changes nothing else.  Layer-major, each launch writes one contiguous block.  Masked entries are exactly 0;
 * rows of padded frames hold what the reference computes for them.
 * The layout branch runs the dense unfused schedule of stlt_forward_attention (the elision flags are ignored), so the logits equal
 * stlt_caf_forward's to fp32 rounding, not bit for bit.  STLT_FLAG_SKIP_PADDING is refused (the maps are those of the padded schedule);
 * so are per_head outside {0, 1}, a workspace below stlt_caf_attention_workspace_bytes, a requested map with more than 1024 keys and an
 * output that is not 4-byte aligned — all STLT_EINVAL, nothing is launched by a refused call.
 * Inference only.  No allocation, no synchronisation; every node of a capture is a kernel (replay: profiles/fusion_attention_bench.md §4).
 * workspace: 256-byte aligned. */
int stlt_caf_forward_attention(const stlt_caf_params* p, const stlt_inputs* in, const float* appearance_features, void* workspace,
                               size_t workspace_bytes, int flags, int per_head, float* logits_caf, float* logits_stlt,
                               float* logits_resnet3d, float* logits_ensemble, const stlt_caf_attention_maps* maps, stlt_stream_t stream);

/* ---- R3D-50 video trunk (reference src/modelling/resnets3d.py:93-214, generate_model(50) minus avgpool / fc; models.py:198-228) ----
 * Internal activations are channels-last (NDHWC).  A Conv3d is an implicit GEMM on the f32 MFMA (csrc/r3d.hip): M = B·To·Ho·Wo
 * output positions, N = c_out, K = kt·kh·kw·c_in, with the weight repacked to (c_out, kt, kh, kw, c_in) by stlt_conv3d_repack.
 * Epilogue, in this order: eval BatchNorm3d from its buffers (γ·(v - mean)/sqrt(var + eps) + β; bn_w == NULL: none), + residual
 * (same NDHWC shape as y; NULL: none), ReLU when relu != 0 — Bottleneck's relu(bn3(conv3(x)) + shortcut), resnets3d.py:70-91.
 * c_in (channels as stored, in x and in the packed weight) must be a multiple of 4: the stem's 3 input channels are padded to 4 by
 * stlt_ncdhw_to_ndhwc / stlt_conv3d_repack.  Padding taps read as zeros.
 * n_split splits the contraction: 1 = whole tiles; > 1 = that many k-ranges, whose partial products go to `workspace`
 * (stlt_conv3d_workspace_bytes(d, n_split) bytes) and are summed in split order by a second launch — deterministic, bit-identical
 * from run to run; 0 = the library's plan for the shape (host arithmetic over the shape alone), split only when the workspace lent
 * holds what the plan needs.  An explicit n_split is a request: the contraction has ceil(K / 32) k-slabs, a request above that is
 * clamped to it, and the ranges are ceil(slabs / n_split) slabs each, so the launch (and the workspace query, which counts the
 * ranges actually launched) can come out below the request.  The data gradient clamps per parity class, and its query is the
 * largest class's need. */
typedef struct {
  int64_t B, T, H, W, c_in;   /* input (B, T, H, W, c_in) NDHWC */
  int64_t c_out;
  int64_t kt, kh, kw;         /* kernel */
  int64_t st, sh, sw;         /* stride */
  int64_t pt, ph, pw;         /* zero padding, each in [0, kernel) */
} stlt_conv3d_desc;
size_t stlt_conv3d_workspace_bytes(const stlt_conv3d_desc* d, int n_split);  /* 0 for a bad descriptor or an unsplit launch */
int stlt_conv3d_fwd(const stlt_conv3d_desc* d, const float* x, const float* w_packed, const float* bn_w, const float* bn_b, const float* bn_mean,
                    const float* bn_var, float bn_eps, const float* residual, int relu, int n_split, void* workspace, size_t workspace_bytes,
                    float* y, stlt_stream_t stream);
/* PyTorch Conv3d weight (c_out, c_in, kt, kh, kw) -> (c_out, kt, kh, kw, c_pad), channels c_in .. c_pad-1 zero */
int stlt_conv3d_repack(const float* w, int64_t c_out, int64_t c_in, int64_t kt, int64_t kh, int64_t kw, int64_t c_pad, float* out, stlt_stream_t stream);
/* layouts: (B, C, T, H, W) -> (B, T, H, W, c_pad) with channels C .. c_pad-1 zero; (B, P, C) -> (B, C, P) */
int stlt_ncdhw_to_ndhwc(const float* x, int64_t B, int64_t C, int64_t T, int64_t H, int64_t W, int64_t c_pad, float* y, stlt_stream_t stream);
int stlt_ndhwc_to_ncdhw(const float* x, int64_t B, int64_t P, int64_t C, float* y, stlt_stream_t stream);
/* MaxPool3d(kernel_size=3, stride=2, padding=1) (resnets3d.py:124) in NDHWC: y (B, To, Ho, Wo, C), To = (T - 1) / 2 + 1 etc.; -inf padding */
int stlt_maxpool3d_ndhwc(const float* x, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, float* y, stlt_stream_t stream);
/* AdaptiveAvgPool3d((1, 1, 1)) of NDHWC (B, P, C) -> (B, C) (Resnet3D's head, models.py:225): positions summed in order, / P */
int stlt_avgpool_ndhwc(const float* x, int64_t B, int64_t P, int64_t C, float* y, stlt_stream_t stream);

/* The whole trunk: the 53 convolutions in state-dict order — the stem (resnet.0 / resnet.1), then per Bottleneck conv1, conv2,
 * conv3 and, in the first block of each layer, downsample.0 (shortcut type B) — each with the BatchNorm3d that follows it. */
#define STLT_R3D_CONVS 53
typedef struct {
  const float* w;             /* packed (c_out, kt, kh, kw, c_in): stlt_conv3d_repack; the stem's c_in padded to 4 */
  const float *bn_w, *bn_b, *bn_mean, *bn_var;
} stlt_r3d_conv;
typedef struct {
  stlt_r3d_conv conv[STLT_R3D_CONVS];
  float bn_eps;               /* 1e-5 */
} stlt_r3d_params;
/* workspace of stlt_r3d_forward for video (B, 3, T, H, W): pure host arithmetic, callable without a GPU; 0 for B <= 0 and for every
 * shape the trunk refuses (T, H or W above 4096, B above 2^20, or one of the 53 convolutions beyond stlt_conv3d_fwd's limits), as
 * stlt_r3d_tape_bytes and stlt_r3d_backward_workspace_bytes: the three come from one plan and are 0 for the same shapes */
size_t stlt_r3d_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W);
/* Resnet3D.forward_features (models.py:221-222) on video (B, 3, T, H, W) NCDHW fp32 -> features (B, 2048, To, Ho, Wo) NCDHW
 * ((B, 2048, 2, 4, 4) for 32 x 112 x 112 clips) and/or pooled (B, 2048), its global average (either may be NULL, not both).
 * BatchNorm in eval semantics always (Resnet3D.train keeps it there, models.py:215-219).  The workspace is 256-byte aligned. */
int stlt_r3d_forward(const stlt_r3d_params* p, const float* video, int64_t B, int64_t T, int64_t H, int64_t W, void* workspace, size_t workspace_bytes,
                     float* features, float* pooled, stlt_stream_t stream);

/* ---- R3D-50 backward (training the trunk; csrc/r3d.hip).  BatchNorm stays eval, so bn(conv(x))'s backward is a per-channel multiply
 * by sc = γ/sqrt(var + eps).  Op level, for the forward conv described by d (x (B, T, H, W, c_in), y (B, To, Ho, Wo, c_out)):
 *   stlt_conv3d_repack_dgrad: torch weight (c_out, c_in, kt, kh, kw) -> the data-gradient copy (as many floats): per parity class of the
 *     stride (s^3 classes, strides 1 or 2, equal in t / h / w), the class's own taps flipped to (c_in, kt', kh', kw', c_out), times
 *     scale[co] (NULL: 1).  Classes without taps take no floats.
 *   stlt_conv3d_bwd_data: dx (B, T, H, W, c_in) = Σ_co dy·w (implicit GEMM over dy, class by class: no zero taps), then
 *     · scale[ci] (NULL: none), + add (dx's shape; NULL: none; may be dx itself), then 0 where mask (dx's shape) <= 0 (NULL: none).
 *     c_out must be a multiple of 4.  n_split as in stlt_conv3d_fwd (0: the library's plan, which needs its workspace).
 *   stlt_conv3d_bwd_weight: dw (c_out, c_in_w, kt, kh, kw) (+)= scale[co] · Σ_m dy[m, co] · x_taps[m, ...]; c_in_w <= c_in drops
 *     padded input channels (the stem's 4th).  The contraction over m splits into ranges whose partials are summed in a fixed order
 *     (n_split 0: the library's plan); the workspace is always needed.  accumulate != 0 adds into dw.
 *   stlt_maxpool3d_ndhwc_train: stlt_maxpool3d_ndhwc that also writes each output's window argmax (0..26, first maximum in scan order);
 *   stlt_maxpool3d_ndhwc_bwd: dx (B, T, H, W, C) from dy and argmax, a deterministic gather, then 0 where mask <= 0 (NULL: none).
 * Every result is bit-identical from run to run.  The two workspace queries return 0 for a descriptor their launch refuses for its
 * shape: a stride above 2 or kt·kh·kw·c_out of 2^31 or more (data gradient), c_out·K above 2^40 floats (weight gradient). */
size_t stlt_conv3d_bwd_data_workspace_bytes(const stlt_conv3d_desc* d, int n_split);
size_t stlt_conv3d_bwd_weight_workspace_bytes(const stlt_conv3d_desc* d, int n_split);
int stlt_conv3d_repack_dgrad(const float* w, const stlt_conv3d_desc* d, const float* scale, float* out, stlt_stream_t stream);
int stlt_conv3d_bwd_data(const stlt_conv3d_desc* d, const float* dy, const float* w_dgrad, const float* scale, const float* mask, const float* add,
                         int n_split, void* workspace, size_t workspace_bytes, float* dx, stlt_stream_t stream);
int stlt_conv3d_bwd_weight(const stlt_conv3d_desc* d, const float* x, const float* dy, const float* scale, int64_t c_in_w, int accumulate, int n_split,
                           void* workspace, size_t workspace_bytes, float* dw, stlt_stream_t stream);
int stlt_maxpool3d_ndhwc_train(const float* x, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, float* y, uint8_t* argmax, stlt_stream_t stream);
int stlt_maxpool3d_ndhwc_bwd(const float* dy, const uint8_t* argmax, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, const float* mask, float* dx,
                             stlt_stream_t stream);

/* Whole trunk.  stlt_r3d_repack_all: ONE launch writing, from the 53 torch weights, every forward copy (fwd[i], as stlt_conv3d_repack)
 * and every data-gradient copy of the 52 non-stem convs (dgrad[i], as stlt_conv3d_repack_dgrad scaled by the conv's BN scale;
 * dgrad[0] is ignored); BN buffers from p (p->conv[i].w is not read).  The shapes are the fixed R3D-50 plan's (the torch weights of
 * conv i in state-dict order); every destination but dgrad[0] must be 16-byte aligned, as the conv kernels read the copies.
 * stlt_r3d_train_forward: stlt_r3d_forward (same outputs, bit for bit, same workspace) that also records the tape: the stem's padded
 * NDHWC input, the stem output, the max-pool output and argmax, and each block's conv1, conv2 and block outputs
 * (stlt_r3d_tape_bytes, pure host arithmetic; 256-byte aligned).
 * stlt_r3d_backward: from the tape and exactly one of dfeatures (B, 2048, To, Ho, Wo) NCDHW or dpooled (B, 2048), writes (accumulate 0)
 * or adds (accumulate != 0) the 53 weight gradients dweight[i] in the torch layout (c_out, c_in, kt, kh, kw).  dgrad_w[i] are the
 * copies of stlt_r3d_repack_all.  This entry point stops at the stem's weight gradient; the video's gradient comes from
 * stlt_r3d_backward_inputs below.  Workspace: stlt_r3d_backward_workspace_bytes. */
size_t stlt_r3d_tape_bytes(int64_t B, int64_t T, int64_t H, int64_t W);
size_t stlt_r3d_backward_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W);
int stlt_r3d_repack_all(const float* const* weights, const stlt_r3d_params* p, float* const* fwd, float* const* dgrad, stlt_stream_t stream);
int stlt_r3d_train_forward(const stlt_r3d_params* p, const float* video, int64_t B, int64_t T, int64_t H, int64_t W, void* workspace, size_t workspace_bytes,
                           void* tape, size_t tape_bytes, float* features, float* pooled, stlt_stream_t stream);
int stlt_r3d_backward(const stlt_r3d_params* p, const float* const* dgrad_w, const void* tape, size_t tape_bytes, int64_t B, int64_t T, int64_t H, int64_t W,
                      const float* dfeatures, const float* dpooled, float* const* dweight, int accumulate, void* workspace, size_t workspace_bytes,
                      stlt_stream_t stream);

/* ---- Pixel gradients: the data gradient of a thin-input convolution (the stem) and the trunk's sweep down to the video ----
 * For the forward conv x (B, T, H, W, 4) NDHWC (c_in <= 4 real channels) -> y (B, To, Ho, Wo, c_out) with kernel 7x7x7, stride
 * (1, 2, 2), padding 3 — the only geometry these entry points take; any other kernel, padding or stride (3 included) and c_in > 4
 * are refused with STLT_EINVAL — one dedicated kernel on v_mfma_f32_16x16x4_f32 (exact f32) writes
 *   dx[b, t, h, w, ci] = Σ_{co, taps} dy · w.
 * A 2x2 block of input positions (h = 2i + a, w = 2j + b) reads one dy window (to in t-3..t+3, ho in i-1..i+2, wo in j-1..j+2), so the
 * 4 (a, b) classes x 4 channels are the 16 columns of the matrix tile and the contraction is 7·4·4·c_out long.
 *   stlt_conv3d_repack_dgrad_thin: torch weight (c_out, c_in <= 4, 7, 7, 7) -> the thin data-gradient copy, times scale[co] (NULL: 1):
 *     [jt 7][jh 4][jw 4][c_out / 4][column 16][4] floats (stlt_conv3d_repack_dgrad_thin_floats(d) = 1792 · c_out; 0 for a refused
 *     descriptor), entry (jt, jh, jw, co / 4, column = (2a + b)·4 + ci, co % 4) = scale[co] · w[co][ci][6 - jt][a + 5 - 2·jh][b + 5 - 2·jw],
 *     and 0 where that tap does not exist (jh = 3 / jw = 3 of the even classes) or ci >= c_in.
 *   stlt_conv3d_bwd_data_thin: dx from dy (16-byte aligned, c_out a multiple of 4) and the thin copy (16-byte aligned).  dx_layout
 *     STLT_DX_NDHWC: (B, T, H, W, 4), the padded channels ci >= c_in STORED as exactly 0; STLT_DX_NCDHW: (B, c_in, T, H, W), the padded
 *     channels not stored at all.  The real channels are the same bits in both.  Taps outside dy read as zero.  Every dx element is
 *     written by one thread in one fixed summation order (no atomics, no workspace): bit-identical from run to run.
 * stlt_r3d_backward_inputs: stlt_r3d_backward with two differences.  dweight == NULL runs the input-only sweep (no weight-gradient
 * launch is enqueued).  dvideo (B, 3, T, H, W) NCDHW, when not NULL, receives the stem's data gradient (stlt_conv3d_bwd_data_thin
 * over the gradient at the stem's output; dgrad_w[0] is the stem's thin copy, made by stlt_conv3d_repack_dgrad_thin with the
 * stem's BN scale γ/sqrt(var + eps)).  dweight and dvideo may not both be NULL.  With dweight given the 53 weight gradients are
 * bit-identical to stlt_r3d_backward's.  Workspace: stlt_r3d_backward_inputs_workspace_bytes (pure host arithmetic; 0 for B <= 0). */
#define STLT_DX_NDHWC 0
#define STLT_DX_NCDHW 1
size_t stlt_conv3d_repack_dgrad_thin_floats(const stlt_conv3d_desc* d);
int stlt_conv3d_repack_dgrad_thin(const float* w, const stlt_conv3d_desc* d, const float* scale, float* out, stlt_stream_t stream);
int stlt_conv3d_bwd_data_thin(const stlt_conv3d_desc* d, const float* dy, const float* w_dgrad_thin, float* dx, int dx_layout, stlt_stream_t stream);
size_t stlt_r3d_backward_inputs_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W);
int stlt_r3d_backward_inputs(const stlt_r3d_params* p, const float* const* dgrad_w, const void* tape, size_t tape_bytes, int64_t B, int64_t T, int64_t H,
                             int64_t W, const float* dfeatures, const float* dpooled, float* const* dweight, int accumulate, float* dvideo,
                             void* workspace, size_t workspace_bytes, stlt_stream_t stream);
/* ---- the trunk's stages, for class activation maps (csrc/r3d.hip; the reductions are further below: Grad-CAM) ----
 * stlt_r3d_layer_geometry: layer 1 .. 4 -> dims[4] = (t, h, w, c) of that stage's output, (B, t, h, w, c) NDHWC on the tape, and the byte
 *     offset of its slot in a stlt_r3d_train_forward tape (the output of the stage's last block, after its ReLU; 256-byte aligned).  Pure
 *     host arithmetic from the trunk's plan, callable without a GPU; STLT_EINVAL for layer outside 1 .. 4, a NULL pointer, and exactly the
 *     shapes stlt_r3d_tape_bytes returns 0 for.
 * stlt_r3d_backward_layer: the reverse sweep of stlt_r3d_backward_inputs with dweight NULL (input-only: no weight-gradient launch), from the
 *     top down to the first block of stage layer + 1, where it stops: dlayer (B, t, h, w, c) NDHWC, 16-byte aligned, receives the gradient
 *     with respect to stage `layer`'s output AFTER its ReLU — the ReLU mask of that output is NOT applied, where the full sweep applies it
 *     because its next consumer wants the pre-ReLU gradient: a hook on layerN's output in the reference's trunk sees the unmasked one, and
 *     Grad-CAM needs that.  layer is 1 .. 3 (stage 4's gradient is the call's own dfeatures / dpooled); tape, dfeatures / dpooled, the
 *     refusals and the workspace (stlt_r3d_backward_workspace_bytes) as stlt_r3d_backward_inputs; dgrad_w[0], the stem's thin copy, is not
 *     read.  The launches above the stop are those of the input-only sweep, with its bits. */
int stlt_r3d_layer_geometry(int64_t B, int64_t T, int64_t H, int64_t W, int layer, int64_t dims[4], size_t* tape_offset);
int stlt_r3d_backward_layer(const stlt_r3d_params* p, const float* const* dgrad_w, const void* tape, size_t tape_bytes, int64_t B, int64_t T, int64_t H,
                            int64_t W, const float* dfeatures, const float* dpooled, int layer, float* dlayer, void* workspace, size_t workspace_bytes,
                            stlt_stream_t stream);

/* ---- training step (reference src/train.py:119-135: forward, loss.backward(); optimiser step further below) ----
 * stlt_train_forward runs every layer on every row — except that the last layer of each tower runs its out-proj /
 * norms / FFN only on the rows read afterwards (CLS row per frame, frame lengths-1 per clip; same loss and gradients,
 * dropout masks keep the rows' original indices) — and records every intermediate the reverse sweep needs in `tape`
 * (fp32; rows padded to a multiple of 32; the caller allocates it ZERO-FILLED once and the library never writes the
 * padding).  stlt_train_backward is the reverse sweep: given dlogits (B, n_classes) it ACCUMULATES (+=) parameter
 * gradients into the buffers named by `grads` — the same struct as the parameters, every pointer being the gradient
 * buffer of that parameter or NULL to skip it (frozen / unused parameters; models.py:172-174).  `scratch` must be
 * zero-filled once by the caller as well.  Embedding rows at padding_idx 0 receive no gradient (models.py:22,91).
 * Dropout (nn.Dropout after both embedding LayerNorms; attention probabilities, dropout1, FFN dropout and dropout2 of
 * every encoder layer — SURVEY.md App. B) is a counter-based mask: with key = splitmix64-finaliser(seed*0x9E3779B97F4A7C15
 * + s*0xD1B54A32D192ED03), element idx of site s is kept iff the keyed 32-bit mixer of csrc/common.h (stlt_keep_k: two
 * multiply-xorshift rounds over idx + key_lo, key_hi folded in between) is >= p*2^32; kept values are scaled by 1/(1-p).
 * The backward recomputes the masks from (p, seed): pass the same values to both calls.  p = 0 disables it.
 * Attention backward supports sequences of up to 256 tokens (the position table).  At most STLT_TRAIN_MAX_CATEGORIES object
 * categories (the embedding-gradient kernel keeps per-category sums in LDS; the reference's vocabularies have 4 and 38):
 * stlt_train_scratch_bytes returns 0 and stlt_train_forward / _backward return STLT_EINVAL above it, before anything runs. */
#define STLT_TRAIN_MAX_CATEGORIES 128
/* stlt_train_backward, when it is given a context, runs the weight-gradient products (off the dX chain) on the context's second stream for
 * the device, forked from and joined to the caller's stream with events inside the call (every exit path, error returns included, joins);
 * without a context, or with this switch at 0, every launch stays on the caller's stream (A/B runs, per-kernel event timing without
 * overlap).  The switch is process-wide; STLT_TRAIN_DW_STREAM in the environment is its initial value (default on);
 * on < 0 goes back to that value.  stlt_get_train_side_stream returns the setting in force (1 / 0), so that a caller can restore it. */
int stlt_set_train_side_stream(int on);
int stlt_get_train_side_stream(void);
size_t stlt_train_tape_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_spatial, int64_t n_temporal);
size_t stlt_train_scratch_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_categories);
/* flags: 0, or STLT_FLAG_SKIP_PADDING (the same value in both calls of a step): forward and reverse sweep run over the
 * real tokens / frames only — same loss and gradients when dropout is off; with dropout the masks are drawn per
 * compacted row, i.e. a different (equally valid) random stream than the padded schedule's.  Each call then
 * synchronises the stream once, unless stlt_inputs carries the batch's exact row counts (n_real_tokens / n_real_frames). */
int stlt_train_forward(const stlt_params* p, const stlt_inputs* in, void* tape, size_t tape_bytes, float* logits,
                       float dropout_p, uint64_t dropout_seed, int flags, stlt_stream_t stream);
int stlt_train_backward(const stlt_params* p, const stlt_params* grads, const stlt_inputs* in, const void* tape,
                        size_t tape_bytes, void* scratch, size_t scratch_bytes, const float* dlogits,
                        float dropout_p, uint64_t dropout_seed, int flags, stlt_ctx* ctx, stlt_stream_t stream);
/* Layout gradients (reference models.py:29-39: batch["boxes"] / batch["scores"] are ordinary autograd leaves there, so a backward on its Stlt
 * gives boxes.grad).  stlt_train_backward_inputs is stlt_train_backward — same arguments, same sweep, stlt_train_backward IS this call with two
 * NULLs — carried one step further: d_boxes (B*T*N*4) and d_scores (B*T*N; NULL, and it must be NULL when the inputs carry no scores) receive
 * the gradient wrt the two inputs.  They are OVERWRITTEN, not accumulated; padded object slots and padded frames hold exactly 0 on both
 * schedules (with STLT_FLAG_SKIP_PADDING every token that is no real row is cleared on the stream).  Both 16-byte aligned; d_scores only with
 * d_boxes.  Works with STLT_FLAG_SKIP_PADDING, STLT_FLAG_TRAIN_BACKBONE and STLT_FLAG_TRAIN_LOWER_ONLY; STLT_EINVAL with
 * STLT_FLAG_TRAIN_UPPER_ONLY (that half never reaches the embedding).  When EVERY member of `grads` is NULL (an input-only sweep: saliency, a
 * frozen model) the sweep enqueues no weight-gradient product, no bias / LayerNorm / embedding-table reduction, and opens no side stream:
 * what is left is the dX chain — the input-gradient products, the LayerNorm / GELU / attention backward — and the kernel below. */
int stlt_train_backward_inputs(const stlt_params* p, const stlt_params* grads, const stlt_inputs* in, const void* tape,
                               size_t tape_bytes, void* scratch, size_t scratch_bytes, const float* dlogits,
                               float dropout_p, uint64_t dropout_seed, int flags, stlt_ctx* ctx, float* d_boxes, float* d_scores,
                               stlt_stream_t stream);

/* ---- attention relevance: which object, in which frame, a prediction rests on (gradient-weighted attention rollout: Chefer, Gur, Wolf,
 * "Generic Attention-model Explainability", 2021).  On the reference this takes need_weights=True on the nn.MultiheadAttention layers of
 * models.py:46-55,118-128, retain_grad on every layer's weights, a backward from the logit and a Python loop over the layers; here every
 * ingredient lies in memory during the input-only reverse sweep: the tape holds each layer's packed QKV, and the gradient wrt the attention
 * core's output (dctx) is in scratch right before the layer's attention backward. ---- */

/* Gradient-weighted attention probabilities of one layer, averaged over the heads:
 *   abar[s,i,j] = (1/H) * sum_h max( P_h[s,i,j] * G_h[s,i,j], 0 ),   G_h[s,i,j] = dctx_h[s,i,:] · v_h[s,j,:]
 * qkv (S*L, 3*H*dh) packed q | k | v, dctx (S*L, H*dh) the gradient wrt the attention core's output, kpm (S*L) bytes (1 = padded key), abar (S, L, L).
 * P_h is exactly what stlt_attn_probs_fwd defines with per_head == 1: the same masks, a masked entry exactly 0, a fully masked row zeros, query
 * rows not filtered by kpm.  G_h is the gradient wrt P_h taken as an independent variable (ctx_h = P_h·V_h, models.py:46-55 through
 * F.multi_head_attention_forward), dropout off.  Every element of abar is written; masked entries are exactly 0.  The heads are summed in
 * their order in registers (no atomics): the same bits on every run.
 * 1 <= L <= 256, 1 <= dh <= 256 (the domain of stlt_attn_core_bwd).  dh == 64 with L <= 64 (every released checkpoint, every layout of the
 * reference) runs on the MFMA kernel of csrc/attn_grad_probs.hip (stlt_attn_probs_fwd's dataflow with a second pair of operands, V and dctx),
 * everything else on its vector-ALU kernel.
 * Alignment: dh % 4 == 0 (16-byte reads, both kernels): qkv and dctx 16 bytes (refused otherwise); other dh: 4 bytes; abar 4 bytes; kpm bytes.
 * Every bad argument is STLT_EINVAL with a message and launches nothing. */
int stlt_attn_grad_probs(const float* qkv, const float* dctx, const uint8_t* kpm, int causal, int64_t S, int64_t L, int64_t H, int64_t dh,
                         float* abar, stlt_stream_t stream);

/* Rollout of the layers' maps through the residual connections: abar (n_layers, S, L, L) -> R (S, L, L),
 *   R_0 = I,   R_l = R_{l-1} + abar_l · R_{l-1}   for l = 1 .. n_layers    (layer 1 is abar[0], the layer next to the input)
 * ONE launch for the whole chain at every length: the columns of R never mix, so a workgroup keeps a block of columns of an item's R in LDS
 * (ping-pong) while the layers stream in from memory — every column for L <= 64 (several items per workgroup when L is small), blocks of 16
 * columns for 64 < L <= 256; no second buffer is needed from the caller at any length.  fp32 FMA over k in ascending order from zero, the old
 * R[i,j] added once, last (an element of R = 1 + 1e-2 keeps 2.5 u over four layers instead of 45 u): the same bits
 * on every run.  n_layers == 0 writes the identity (abar may then be NULL).  0 <= n_layers <= 64, 1 <= L <= 256; abar, R 4 bytes.
 * Every bad argument is STLT_EINVAL with a message and launches nothing. */
int stlt_attn_rollout(const float* abar, int64_t n_layers, int64_t S, int64_t L, float* R, stlt_stream_t stream);

/* Relevance of object slot n of frame t for clip b's prediction:
 *   rel[b,t,n] = r_temporal[b, lengths[b]-1, t] * r_spatial[b,t,0,n]
 * r_temporal (B, T, T) and r_spatial (B*T, N, N) are the two towers' rollouts.  Row 0 of a frame is its CLS token, the row the frames embedding
 * reads (models.py:79); row lengths[b]-1 of a clip is the frame the head reads (models.py:189-192).  rel (B, T, N); a length outside
 * 1 ... T makes the clip's entries NaN (the convention of stlt_loss_fwd_bwd).  Pointers 4 bytes, lengths (int64) 8; STLT_EINVAL otherwise. */
int stlt_relevance_combine(const float* r_temporal, const float* r_spatial, const int64_t* lengths, int64_t B, int64_t T, int64_t N, float* rel,
                           stlt_stream_t stream);

typedef struct {
  float *abar_spatial;     /* (n_spatial, B*T, N, N): every spatial layer's gradient-weighted map; NULL only when n_spatial == 0 */
  float *abar_temporal;    /* (n_temporal, B, T, T); NULL only when n_temporal == 0 */
  float *rollout_spatial;  /* (B, T, N, N) */
  float *rollout_temporal; /* (B, T, T)    */
  float *relevance;        /* (B, T, N)    */
} stlt_relevance_maps;

/* The relevance of the objects of a batch for the objective whose gradient wrt the logits is `dlogits` (stlt_saliency_seed: one raw logit per
 * clip), on the tape of a stlt_train_forward with dropout 0: the arguments of stlt_train_backward_inputs without the gradient table and
 * without d_boxes / d_scores, plus the sinks.  It runs the input-only sweep (no weight-gradient product, no parameter reduction, no side
 * stream) with one stlt_attn_grad_probs launch on (the layer's packed QKV, dctx) immediately before each attention backward, stops once the
 * first spatial layer's map is written (the layer-0 input product and the embedding backward are not needed), then launches the two rollouts
 * and the combine.  All five maps are overwritten.  Entries of padded frames and padded object slots of `relevance` are exactly 0: a padded key's
 * column of every abar is 0 and the temporal mask is causal, so the rollouts' entries that the combine reads there are sums of exact zeros.
 * In the last layer of a tower only the rows that are read afterwards (the CLS rows / frame lengths-1) carry a gradient: the other rows of that
 * layer's abar are exactly 0, as autograd has them.
 * With STLT_FLAG_TRAIN_BACKBONE (the layout branch of a fusion model, on the tape of a stlt_train_forward with that flag) `dlogits` is the
 * (B, T, d) gradient of the backbone's output, as in stlt_train_backward; the per-layer maps and the two rollouts are written, and
 * maps->relevance must be NULL: stlt_relevance_combine_joint reads the rollouts out for the fusion models.
 * STLT_EINVAL before any launch: STLT_FLAG_SKIP_PADDING (the maps have the padded geometry), dropout_p != 0, STLT_FLAG_TRAIN_UPPER_ONLY /
 * _LOWER_ONLY, N or T above 256, a NULL or misaligned (4 bytes) map, a relevance map given with _BACKBONE.  tape / scratch: as stlt_train_backward.
 * No allocation, no synchronisation, capturable.  Profiling: the maps under STLT_K_ATTN_PROBS, rollouts and combine under STLT_K_MISC. */
int stlt_train_backward_relevance(const stlt_params* p, const stlt_inputs* in, const void* tape, size_t tape_bytes, void* scratch,
                                  size_t scratch_bytes, const float* dlogits, float dropout_p, uint64_t dropout_seed, int flags, stlt_ctx* ctx,
                                  const stlt_relevance_maps* maps, stlt_stream_t stream);

/* ---- attention relevance of the fusion models (CAF / CACNF / LCF): how much of a class decision came through the video tokens and how much
 * through the layout.  T layout frames and A = app_tokens + 1 appearance tokens (token 0 is the CLS token, models.py:247-262) form one stacked
 * token set of J = T + A: joint index t is frame t, joint index T + a is appearance token a.  This is the bi-modal rule of Chefer, Gur, Wolf,
 * "Generic Attention-model Explainability for Interpreting Bi-Modal and Encoder-Decoder Transformers" (ICCV 2021) without its row
 * normalisation: the rule of stlt_attn_rollout continued over two token sets. ---- */

/* stlt_attn_grad_probs for queries and keys that lie in different buffers and differ in number — the CrossAttentionLayer of the fusion models
 * (models.py:362-382, called at 411-419):
 *   abar[s,i,j] = (1/H) * sum_h max( P_h[s,i,j] * G_h[s,i,j], 0 ),   G_h[s,i,j] = dctx_h[s,i,:] · v_h[s,j,:]
 * q rows ldq floats apart ((S*Lq) rows), k and v rows ldkv floats apart ((S*Lk) rows); only the first H*dh columns of each are read.  A cross
 * block's buffers: q (S*Lq, d), the packed kv (S*Lk, 2d) as k = kv, v = kv + d, ldkv = 2d; a packed self block's: q = qkv, k = qkv + d,
 * v = qkv + 2d, ldq = ldkv = 3d.  dctx (S*Lq, H*dh), abar (S, Lq, Lk).  P_h is exactly what stlt_attn_probs_cross_fwd defines with
 * per_head == 1: the same masks (kpm: (S*Lk) bytes over the key tokens, never NULL; causal requires Lq == Lk), a masked entry exactly 0, a
 * fully masked row zeros.  Every element of abar is written; the heads are summed in their order in registers: the same bits on every run.
 * 1 <= Lq, Lk <= 256, 1 <= dh <= 256 (the domain of stlt_attn_bwd).  dh == 64 with Lk <= 64 (any Lq: every fusion block of the reference's
 * shapes) runs on the MFMA kernel of csrc/attn_grad_probs.hip and needs q, k, v and dctx 16-byte aligned and ldq, ldkv multiples of 4
 * (refused otherwise); everything else on its vector-ALU kernel, pointers and strides 4 bytes.  abar 4 bytes; kpm bytes.  Routed by what was
 * measured (profiles/fusion_relevance_bench.md): an MFMA shape with more than 32 keys and fewer than 128 work units, S * ceil(Lq / 16), also
 * runs on the vector-ALU kernel — the same contract and refusals, results equal to fp32 rounding.
 * Every bad argument is STLT_EINVAL with a message and launches nothing. */
int stlt_attn_grad_probs_cross(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* dctx, const uint8_t* kpm,
                               int causal, int64_t S, int64_t Lq, int64_t Lk, int64_t H, int64_t dh, float* abar, stlt_stream_t stream);

/* Rollout over the stacked token set: R (S, J, J),
 *   R_0 = blockdiag(r_layout (S,T,T), r_appearance (S,A,A))        (a NULL pointer: the identity block)
 * and for fusion layer l = 1 .. n_fusion (CrossModalModule.forward, models.py:403-431) three steps R <- R + X·R:
 *   1. X = [[0, l2a_l], [a2l_l, 0]]                  both cross blocks read the layer's input: one simultaneous step (411-419)
 *   2. X = blockdiag(f_layout_l, f_appearance_l[0])  layout_attn and appearance_attn (421-427)
 *   3. X = blockdiag(0, f_appearance_l[1])           appearance_ffn, a SelfAttentionLayer (models.py:401); layout_ffn has no attention
 * The maps have the geometry of stlt_caf_attention_maps: layout_to_appearance (n, S, T, A), appearance_to_layout (n, S, A, T), fusion_layout
 * (n, S, T, T), fusion_appearance (n, 2, S, A, A).  Only the non-zero quadrants are read.  ONE launch for the whole chain: the columns of R
 * never mix, so a workgroup keeps 16 columns of one item's R in LDS (ping-pong, 64 KB at J = 512) while the maps stream in from memory.
 * fp32 FMA over k in ascending order from zero, the old R[i,j] added once, last: the same bits on every run.  n_fusion == 0 (LCF) writes the block-diagonal (the maps may be NULL).
 * 0 <= n_fusion <= 64, 1 <= T, A <= 256; every pointer 4 bytes.  Every bad argument is STLT_EINVAL with a message and launches nothing. */
int stlt_attn_rollout_joint(const float* r_layout, const float* r_appearance, const float* layout_to_appearance, const float* appearance_to_layout,
                            const float* fusion_layout, const float* fusion_appearance, int64_t n_fusion, int64_t S, int64_t T, int64_t A, float* R,
                            stlt_stream_t stream);

/* The read-out of a fusion model's head: row[b,:] = w_layout * R[b, lengths[b]-1, :] + w_appearance * R[b, T, :] — the frame the layout head
 * reads (models.py:189-192) and the appearance CLS token (models.py:260-262); (1,0) for the "stlt" head, (0,1) for "resnet3d", (1,1) for "caf",
 * "lcf" and "ensemble" (models.py:486-498, 520-549).
 *   frame_rel[b,t] = row[b,t]     app_rel[b,a] = row[b,T+a]     rel[b,t,n] = frame_rel[b,t] * r_spatial[b,t,0,n]
 * R (B, J, J), r_spatial (B*T, N, N) the spatial tower's rollout; rel (B, T, N), frame_rel (B, T), app_rel (B, A).  A length outside 1 ... T
 * makes all three outputs of that clip NaN (the convention of stlt_relevance_combine).  Pointers 4 bytes, lengths (int64) 8; STLT_EINVAL otherwise. */
int stlt_relevance_combine_joint(const float* R, const float* r_spatial, const int64_t* lengths, int64_t B, int64_t T, int64_t A, int64_t N,
                                 float w_layout, float w_appearance, float* rel, float* frame_rel, float* app_rel, stlt_stream_t stream);

/* ---- optimiser step of the training loop (reference train.py:128-131 with utils/train_inference_utils.py:37-54) ----
 * The reverse sweep writes all parameter gradients into ONE flat fp32 buffer (what a data-parallel run all-reduces).
 * stlt_grad_norm: out[0] = ||g||_2 over the n floats, out[1] = min(1, max_norm / (out[0] + 1e-6)) — the factor
 * torch.nn.utils.clip_grad_norm_ scales the gradients by (max_norm <= 0: out[1] = 1).  scratch: >= 1024 floats.
 * stlt_adamw_step: torch.optim.AdamW.step (decoupled weight decay, bias correction, fp32) over a device table of
 * chunks; element i of a chunk is parameter param[i], its gradient flat_grad[flat_offset + i] (scaled by
 * norm_and_clip[1] when given) and its moments exp_avg / exp_avg_sq at the same flat offset.  step counts from 1.  lr, beta1, beta2 and
 * eps are doubles, as torch holds them: 1 - beta2 taken from a beta2 already rounded to fp32 is off by 1.3e-5 of its value (0.999), and
 * with it every increment of exp_avg_sq. */
typedef struct {
  float* param;
  int64_t flat_offset;
  int32_t n;
  float weight_decay;
} stlt_opt_chunk;
/* ---- per-kernel backward entry points (autograd of the K-row forwards above; the fusion models' training is composed
 * from these, the STLT training step uses the fixed reverse sweep of stlt_train_backward) ----
 * Alignment: stlt_linear_bwd — dy, db and the scratch 16 bytes (refused otherwise: the column sums move 16 bytes per lane); x, w, dx, dw
 *   none beyond 4 bytes (its three products route them as stlt_gemm does).  stlt_add_layernorm_bwd, stlt_embed_bwd, stlt_frames_embed_bwd —
 *   every float pointer and the scratch 16 bytes (refused otherwise, the message names the pointer).  stlt_attn_core_bwd / stlt_attn_bwd
 *   (and stlt_attn_fwd_dropout) with dh == 64 likewise (masks are bytes); with any other dh the activations and gradients none beyond 4
 *   bytes (in_proj_b_grad and its scratch: 16).  Index arrays 8 bytes.  Every scratch is used inside
 *   exactly the bytes its *_scratch_bytes function returns.
 * stlt_linear_bwd: y = x·Wᵀ + b (no activation).  dx (M,K) = dy·W (nullable), dw (N,K) += dyᵀ·x (nullable), db (N) +=
 *   column sums of dy (nullable).  scratch: stlt_linear_bwd_scratch_bytes(N).  ctx (nullable): dx may run on the context's transposed copy of w.
 * stlt_attn_bwd: backward of stlt_attn_cross_fwd (and, with q = qkv, k = qkv+d, v = qkv+2d, of stlt_attn_core_fwd):
 *   dq / dk / dv written (not accumulated) with their own leading dimensions; sequences of at most 256 tokens on either
 *   side (above 64 a streamed variant: query tiles of 32, keys / values in tiles through LDS); head dims other than 64: attn_any.hip.
 * stlt_add_layernorm_bwd: out = LN_eps(x + res)·w + b.  ds = gradient wrt the sum (the gradient of both x and res);
 *   g_w / g_b accumulate (nullable).  scratch: stlt_add_layernorm_bwd_scratch_bytes(d).
 * stlt_gelu_fwd / stlt_gelu_bwd: exact-erf GELU and du = dh * gelu'(u), n a multiple of 4. */
size_t stlt_linear_bwd_scratch_bytes(int64_t N);
int stlt_linear_bwd(const float* x, const float* w, const float* dy, int64_t M, int64_t N, int64_t K, float* dx, float* dw, float* db,
                    stlt_ctx* ctx, void* scratch, size_t scratch_bytes, stlt_stream_t stream);
/* Backward of K3 on the packed projection (what the training sweep runs per layer): dqkv (S*L, 3*H*dh) from qkv and dctx, with
 * the masks of stlt_attn_core_fwd, optional dropout of the probabilities (site as in stlt_train_forward) and, when in_proj_b_grad
 * is not NULL, in_proj_b_grad (3*H*dh) += column sums of dqkv.  dh == 64, L <= 64: v_mfma_f32_16x16x4_f32 tiles (one wave per
 * sequence and head); up to 256: plain FMA, keys streamed through LDS.  Any other head dim (1 ... 256): the two-phase vector-ALU
 * kernel of csrc/attn_any.hip (L <= 256, no atomics).  scratch: stlt_attn_core_bwd_scratch_bytes(H) bytes. */
size_t stlt_attn_core_bwd_scratch_bytes(int64_t H);
int stlt_attn_core_bwd(const float* qkv, const float* dctx, const uint8_t* kpm, int causal, int64_t S, int64_t L, int64_t H, int64_t dh,
                       float dropout_p, uint64_t seed, uint32_t site, float* dqkv, float* in_proj_b_grad, void* scratch, size_t scratch_bytes,
                       stlt_stream_t stream);
/* attention with train-mode dropout of the probabilities (nn.MultiheadAttention(dropout=p)): counter-based mask from
 * (seed, site, query row, head, key position); stlt_attn_bwd given the same (p, seed, site) recomputes it.  p = 0: none. */
int stlt_attn_fwd_dropout(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const uint8_t* kpm, int causal,
                          int64_t S, int64_t Lq, int64_t Lk, int64_t H, int64_t dh, float dropout_p, uint64_t seed, uint32_t site, float* ctx,
                          stlt_stream_t stream);
int stlt_attn_bwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* dctx, const uint8_t* kpm,
                  int causal, int64_t S, int64_t Lq, int64_t Lk, int64_t H, int64_t dh, float dropout_p, uint64_t seed, uint32_t site,
                  float* dq, int64_t lddq, float* dk, float* dv, int64_t lddkv, stlt_stream_t stream);
size_t stlt_add_layernorm_bwd_scratch_bytes(int64_t d);
int stlt_add_layernorm_bwd(const float* dy, const float* x, const float* res, const float* ln_w, float eps, int64_t M, int64_t d,
                           float* ds, float* g_w, float* g_b, void* scratch, size_t scratch_bytes, stlt_stream_t stream);
int stlt_gelu_fwd(const float* u, float* h, int64_t n, stlt_stream_t stream);  /* h = gelu(u) (exact erf form); n % 4 == 0; u, h 16 bytes (refused otherwise) */
/* K1 / K7 for an op-level autograd: the forward also returns the pre-LayerNorm sum; the LayerNorm part of the backward is
 * stlt_add_layernorm_bwd on that sum (res = NULL), the rest is below: given d_pre (gradient wrt the sum) the parameter
 * gradients ACCUMULATE into g_* (nullable); the gradient wrt the K7 input rows is d_pre itself.  Row 0 of the category /
 * frame-type tables is the padding index and receives none (models.py:22,91). */
int stlt_embed_fwd_train(const int64_t* categories, const float* boxes, const float* scores, const float* cat_table, int64_t n_categories,
                         const float* box_w, const float* box_b, const float* score_w, const float* score_b, const float* ln_w,
                         const float* ln_b, float eps, int64_t n_tokens, int64_t d, float* pre_out, float* out, stlt_stream_t stream);
size_t stlt_embed_bwd_scratch_bytes(int64_t n_tokens, int64_t n_categories, int64_t d);
int stlt_embed_bwd(const float* d_pre, const int64_t* categories, const float* boxes, const float* scores, int64_t n_categories,
                   int64_t n_tokens, int64_t d, float* g_cat, float* g_box_w, float* g_box_b, float* g_score_w, float* g_score_b,
                   void* scratch, size_t scratch_bytes, stlt_stream_t stream);
/* K1's gradient wrt its inputs (models.py:29-39: the sum is category row + box_embedding(boxes) + score_embeddings(scores)): given d_pre
 * (n_tokens, d), d_boxes[t][j] = sum_c d_pre[t][c] * box_w[c][j] (box_w (d,4) as nn.Linear(4, d) stores it) and d_scores[t] = sum_c
 * d_pre[t][c] * score_w[c] (score_w (d,1)).  Outputs are overwritten; the summation order is fixed (two calls are bit-identical).
 * d_scores and score_w are NULL together.  STLT_EINVAL before any launch: a NULL required pointer, d % 4 != 0 (or d > 2048), n_tokens < 0,
 * any pointer off a 16-byte boundary. */
int stlt_embed_bwd_inputs(const float* d_pre, const float* box_w, const float* score_w, int64_t n_tokens, int64_t d, float* d_boxes,
                          float* d_scores, stlt_stream_t stream);
int stlt_frames_embed_fwd_train(const float* spatial, int64_t row_stride, const int64_t* frame_types, const float* pos_table,
                                const float* type_table, const float* ln_w, const float* ln_b, float eps, int64_t B, int64_t T, int64_t d,
                                float* pre_out, float* out, stlt_stream_t stream);
size_t stlt_frames_embed_bwd_scratch_bytes(int64_t T, int64_t d);
int stlt_frames_embed_bwd(const float* d_pre, const int64_t* frame_types, int64_t B, int64_t T, int64_t d, float* g_pos, float* g_type,
                          void* scratch, size_t scratch_bytes, stlt_stream_t stream);
int stlt_gelu_bwd(const float* dh, const float* u, float* du, int64_t n, stlt_stream_t stream);  /* du = dh * gelu'(u); n % 4 == 0; dh, u, du 16 bytes (refused otherwise) */
/* Element-wise pieces of the op-level training path.  stlt_dropout: y[i] = keep(seed, site, i) ? x[i] / (1-p) : 0 with the
 * library's counter-based mask — the backward is the same call on the gradient (nn.Dropout at models.py:333-376 and inside
 * nn.TransformerEncoderLayer).  stlt_relu_bwd: dx = dy where the activation's OUTPUT y is positive (the ReLU itself runs in
 * the producing product's epilogue: stlt_linear_fwd with STLT_ACT_RELU).  Any n; every buffer 16-byte aligned (refused otherwise, the
 * message names it); y may alias x / dx may alias dy. */
int stlt_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, uint32_t site, stlt_stream_t stream);
int stlt_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, stlt_stream_t stream);

/* Criterion of the reference (utils/train_inference_utils.py:64-76) and its gradient in one pass: loss_out[0] = weight *
 * mean loss, dlogits = weight * d(mean loss)/d(logits).  CROSS_ENTROPY: labels int64 (B); BCE_WITH_LOGITS: labels float
 * (B,K) multi-hot.  `weight` = 1 / number of logit heads (the reference averages the heads' losses).  scratch: >= B floats.
 * Alignment: none beyond the element types' (scalar accesses).  stlt_grad_norm: flat_grad 16 bytes (refused otherwise).  stlt_adamw_step:
 * none beyond 4 bytes — a chunk whose parameter, gradient and moment pointers are all 16-byte aligned moves 16 bytes per lane, any other
 * chunk one float at a time, same arithmetic. */
#define STLT_LOSS_CROSS_ENTROPY 0
#define STLT_LOSS_BCE_WITH_LOGITS 1
int stlt_loss_fwd_bwd(const float* logits, const void* labels, int kind, int64_t B, int64_t K, float weight,
                      float* scratch, float* loss_out, float* dlogits, stlt_stream_t stream);
/* Seed of a saliency pass (the gradient of one raw logit per clip, what `logits[b, k].backward()` starts from on the reference's Stlt,
 * models.py:166-195): dlogits (B,K) row b = e_k with k = target[b] (int64), or, with target == NULL, the argmax of logits row b (lowest
 * index on ties).  An out-of-range target makes the row NaN, the convention of stlt_loss_fwd_bwd.  logits may be NULL when target is given. */
int stlt_saliency_seed(const float* logits, const int64_t* target, int64_t B, int64_t K, float* dlogits, stlt_stream_t stream);
int stlt_grad_norm(const float* flat_grad, int64_t n, float max_norm, float* scratch, float* out, stlt_stream_t stream);
int stlt_adamw_step(const stlt_opt_chunk* chunks_dev, int64_t n_chunks, const float* flat_grad, float* exp_avg, float* exp_avg_sq,
                    const float* norm_and_clip, double lr, double beta1, double beta2, double eps, int64_t step, stlt_stream_t stream);

/* ---- block-level training calls for the fusion models (CAF / CACNF / LCF; reference models.py:328-431, 239-246) ----
 * One native forward and one native reverse call per residual block, so an optimisation step of a fusion model is a few
 * dozen calls instead of a few hundred op-level ones.  The caller owns the tape tensors (q / kv / ctx / a, u / h / f) and the
 * two backward buffers (stlt_block_keep_bytes / stlt_block_work_bytes, below).
 *   attention block (SelfAttentionLayer / CrossAttentionLayer :345-382, and the first half of nn.TransformerEncoderLayer):
 *     out = LN_eps(x + drop(MHA(x, c, c) Wo^T + bo)); c == NULL: self-attention on a packed q|k|v buffer q (S*Lq, 3d);
 *     else q (S*Lq, d) and kv (S*Lk, 2d).  kpm (S*Lk) bytes over the keys (never NULL: pass zeros).  Dropout sites: site0 =
 *     attention probabilities, site0 + 1 = in front of the residual.
 *   feed-forward block (:384-401 layout_ffn, and the second half of nn.TransformerEncoderLayer):
 *     out = LN_eps(x + drop(W2 drop_inner(act(W1 x + b1)) + b2)), act = STLT_ACT_GELU (u and h kept) or STLT_ACT_RELU (h kept);
 *     inner_dropout != 0 applies site0 to the hidden, site0 + 1 is the dropout in front of the residual.
 * gemm_scratch (forward calls): NULL, or stlt_gemm_scratch_bytes() of device memory lent for the call's stream-K launches.
 * The backward calls ACCUMULATE (+=) into the gradient struct's buffers (NULL members are skipped), write dx (and dc, the
 * gradient wrt the context tokens of a cross-attention block), and recompute the dropout masks from (drop_p, seed, site0). */
/* Deferred weight gradients of the block calls.  After stlt_ctx_dw_defer(ctx, 1) the *_block_bwd_train calls that name `ctx` queue their
 * weight-gradient products (g_w += dyᵀ·x) in the context instead of launching them; stlt_ctx_dw_flush runs the queue as grouped stream-K
 * launches of up to 32 products on `stream` (the stream the blocks ran on) with stlt_gemm_scratch_bytes() of scratch, in queue order (two
 * products into the same gradient never share a launch).  The CALLER keeps every operand of the queued products alive and unchanged until the
 * flush: the blocks' `keep` buffers (they hold the output gradients) and the forward activations the blocks were handed — their `work`
 * buffers are free again when the call returns.  mode 0 stops collecting (queued products stay), -1 stops and discards.  The queue holds at
 * most 512 products: a block that would overflow it launches its own.  A training step of the fusion models (models.py:403-431) makes 34
 * block calls.  torch's autograd engine runs the block backwards on its own thread: the queue follows the handle, not the thread. */
int stlt_ctx_dw_defer(stlt_ctx* ctx, int mode);
int stlt_ctx_dw_pending(stlt_ctx* ctx);
int stlt_ctx_dw_flush(stlt_ctx* ctx, void* gemm_scratch, size_t gemm_scratch_bytes, stlt_stream_t stream);
/* Transposed weight copies for the input-gradient products of a training step (csrc/wt_cache.hip).  dX = dY·W with W (n_out, k_in) read as
 * it lies runs 13 - 17 % below a forward product of the same shape on the small-tile kernel; with a copy wt (k_in, n_out) it IS a forward
 * product.  stlt_ctx_wt_refresh writes every entry's copy (wt[k][n] = w[n][k]; caller-owned buffers; dimensions multiples of 4, 16-byte
 * aligned) on `stream` and makes the set current in `ctx`: until stlt_ctx_wt_clear, every input-gradient product of a call that names
 * `ctx` on the same device (stlt_train_backward, the block backwards, stlt_linear_bwd, stlt_input_grad_small with tile 0) whose weight
 * pointer lies inside a registered weight — row ranges of a packed in-projection starting at a multiple of four rows included — and that
 * routes to the small tiles reads the copy.  The library orders each such call's stream behind the transposes.  The caller refreshes after
 * the weights changed (train.Trainer: at the start of every step) and clears before anything else may change them (at the end of the
 * step); a call that names another context, or none, never sees a copy.  stlt_ctx_wt_hits: products LAUNCHED on a copy so far. */
typedef struct {
  const float* w;      /* (n_out, k_in) row-major: nn.Linear's weight */
  float* wt;           /* (k_in, n_out) row-major: the copy */
  int64_t n_out, k_in;
} stlt_wt_entry;
int stlt_ctx_wt_refresh(stlt_ctx* ctx, const stlt_wt_entry* entries, int64_t n, stlt_stream_t stream);
int stlt_ctx_wt_clear(stlt_ctx* ctx);
long long stlt_ctx_wt_hits(stlt_ctx* ctx);
/* Device memory of a block backward, in two buffers: `keep` (stlt_block_keep_bytes(rows, d, kind); kind 0 = attention block, 1 =
 * feed-forward block; rows = the larger token count of the block) holds the gradients the block's weight-gradient products read — with
 * deferral on it must stay untouched until the flush, one buffer per block call; `work` (stlt_block_work_bytes(rows, d): stream-K partial
 * tiles, reduction pools, a context gradient) is dead when the call has enqueued its launches — one buffer per stream serves all blocks. */
size_t stlt_block_keep_bytes(int64_t rows, int64_t d, int kind);
size_t stlt_block_work_bytes(int64_t rows, int64_t d);
int stlt_attn_block_fwd_train(const stlt_attn_block_params* p, int64_t d, int64_t H, float eps, const float* x, int64_t Lq, const float* c,
                              int64_t Lk, const uint8_t* kpm, int causal, int64_t S, float drop_p, uint64_t seed, uint32_t site0, float* q,
                              float* kv, float* ctx, float* a, float* out, void* gemm_scratch, size_t gemm_scratch_bytes, stlt_stream_t stream);
int stlt_attn_block_bwd_train(const stlt_attn_block_params* p, const stlt_attn_block_params* g, int64_t d, int64_t H, float eps, const float* x,
                              int64_t Lq, const float* c, int64_t Lk, const uint8_t* kpm, int causal, int64_t S, float drop_p, uint64_t seed,
                              uint32_t site0, const float* q, const float* kv, const float* ctx, const float* a, const float* dy, float* dx,
                              float* dc, stlt_ctx* tctx, void* keep, size_t keep_bytes, void* work, size_t work_bytes, stlt_stream_t stream);
/* The input-only reverse call of an attention block for the fusion models' relevance (SelfAttentionLayer / CrossAttentionLayer, models.py:
 * 345-382): stlt_attn_block_bwd_train with every member of `g` NULL, drop_p == 0 and no context — the same buffers, the same launches, dx and
 * dc the same bits — plus ONE launch right before the attention backward, on what lies in memory there (the block's q | kv and the gradient
 * wrt the attention core's output): stlt_attn_grad_probs for a packed self block (c == NULL), stlt_attn_grad_probs_cross otherwise, into
 * abar (S, Lq, Lk).  Lq, Lk <= 256; abar 4 bytes, q and kv 16 bytes; refused (STLT_EINVAL) before any launch otherwise. */
int stlt_attn_block_bwd_relevance(const stlt_attn_block_params* p, int64_t d, int64_t H, float eps, const float* x, int64_t Lq, const float* c,
                                  int64_t Lk, const uint8_t* kpm, int causal, int64_t S, const float* q, const float* kv, const float* ctx,
                                  const float* a, const float* dy, float* dx, float* dc, float* abar, void* keep, size_t keep_bytes, void* work,
                                  size_t work_bytes, stlt_stream_t stream);
int stlt_ffn_block_fwd_train(const stlt_ffn_block_params* p, int64_t d, float eps, int act, int inner_dropout, const float* x, int64_t M,
                             float drop_p, uint64_t seed, uint32_t site0, float* u, float* h, float* f, float* out, void* gemm_scratch,
                             size_t gemm_scratch_bytes, stlt_stream_t stream);
int stlt_ffn_block_bwd_train(const stlt_ffn_block_params* p, const stlt_ffn_block_params* g, int64_t d, float eps, int act, int inner_dropout,
                             const float* x, int64_t M, float drop_p, uint64_t seed, uint32_t site0, const float* u, const float* h, const float* f,
                             const float* dy, float* dx, stlt_ctx* tctx, void* keep, size_t keep_bytes, void* work, size_t work_bytes, stlt_stream_t stream);

/* ---- evaluators on the device (reference src/utils/evaluation.py) ----
 * stlt_eval_topk: EvaluatorSomething.process (evaluation.py:21-34) for one logit head.  counts[0] += clips whose label is
 * the arg-max, counts[1] += clips whose label is among the five largest logits (int64 device counters, accumulated with
 * integer atomics).  The label's rank is the number of classes with a larger logit, or an equal logit at a lower index.
 * stlt_eval_average_precision: map() + the empty-clip rule of charades_map (evaluation.py:100-131).  scores / truths are
 * (n, C) row-major float (scores = sigmoid of the logits, truths multi-hot); ap[c] = average precision of class c (NaN
 * when the class has no positive), positives[c] = its number of positives; scratch >= n bytes.  n <= stlt_eval_max_clips()
 * (a class column is sorted inside one workgroup's LDS).  Equal scores keep clip order (the reference's argsort leaves
 * ties unspecified).
 * Alignment (all three evaluator calls): none beyond the element types' (floats 4, int64 / double 8); logits rows of `ld` floats are read
 * in their first K / C columns only; stlt_eval_store_sigmoid writes rows [row0, row0 + B) of the tables and nothing else. */
int stlt_eval_topk(const float* logits, int64_t ld, const int64_t* labels, int64_t B, int64_t K, int64_t* counts,
                   stlt_stream_t stream);
int64_t stlt_eval_max_clips(void);
/* EvaluatorActionGenome.process (evaluation.py:76-82) for one batch: pred[i][c] = (double)sigmoid_f32(logits[i][c]) and
 * truth[i][c] = (double)labels[i][c] written into rows [row0, row0 + B) of the two (total, C) float64 device tables. */
int stlt_eval_store_sigmoid(const float* logits, int64_t ld, const float* labels, int64_t B, int64_t C, double* pred, double* truth,
                            int64_t row0, stlt_stream_t stream);
int stlt_eval_average_precision(const float* scores, const float* truths, int64_t n, int64_t C, double* ap, double* positives,
                                uint8_t* scratch, stlt_stream_t stream);

/* ---- the perturbation test of an attribution map (csrc/perturb.hip; Chefer, Gur, Wolf 2021) ----
 * Rank the real object tokens of every clip by a map, delete the first k of them for a rising k, score the logits of every reduced batch.
 * All three calls are stream-ordered, allocate nothing, read nothing back and are capturable in a hipGraph; a bad extent or a NULL required
 * pointer is STLT_EINVAL with a message and launches nothing.  Alignment: none beyond the element types' (floats / int32 4, int64 8): every
 * access is one element wide.  Only the logical extents are touched.
 *
 * stlt_perturb_rank: the removal order of each clip.  scores (B,T,N) for unit STLT_PERTURB_OBJECT, (B,T) for STLT_PERTURB_FRAME; kpm_boxes
 * (B,T,N) src_key_padding_mask_boxes; lengths (B,).  Candidates of clip b — object: slots (t,n) with t < lengths[b]-1 (never the extract frame
 * the dataset appends, datasets.py:97-113), n >= 1 (never the CLS slot, datasets.py:70-72) and mask 0; frame: frames t < lengths[b]-1 that hold
 * at least one such slot.  Order: by score, descending (1) or ascending (0), compared as floats with -0 == +0; ties go to the lower flat
 * index (t*N+n, or t) in both orders; NaN is removed last in both orders.  rank (same shape as scores, int32) = position in the removal order
 * (0 = first) for candidates, -1 elsewhere; n_candidates (B,) int32.  One workgroup per clip sorts packed 64-bit keys in LDS, so
 * T*N <= stlt_perturb_max_items() (16384) for both units; beyond it STLT_EINVAL.
 *
 * stlt_perturb_apply: the batch `in` (stlt_inputs: B, T, N and the seven tensors; scores may be NULL; the row counts are not read) with the
 * first k candidates deleted, for every step s in [s0, s1], 0 <= s0 <= s1 <= steps, steps >= 1: k = floor(s * n_candidates[b] / steps)
 * (64-bit product).  The (s1-s0+1)*B output clips are step-major: clip (s-s0)*B + b is clip b at step s.  Deleted are the candidates with
 * 0 <= rank < k — for unit frame every slot n >= 1 with mask 0 of the frames with rank < k.  A deleted slot is what the reference's dataset
 * and collater make of a slot without a detection (datasets.py:88-93, 274-278): category 0, box (0,0,0,0), score 0 (when the batch has
 * scores), mask 1.  Everything else is copied bit for bit: the kept slots, lengths, kpm_frames and the frame types — except that a frame
 * t < lengths[b]-1 that had a real slot and has none left gets empty_frame_type (frame2type["empty"], datasets.py:64-69).  Slots are not
 * compacted.  rank and n_candidates must be what stlt_perturb_rank wrote for this very batch and unit (rank's shape tells the unit's); they are
 * trusted, not checked: other values delete other slots, inside the extents all the same.  removed (steps+1, B) int32: rows s0 .. s1 receive k; the other rows are not touched.  Step 0 reproduces the input, step
 * `steps` deletes every candidate.  The outputs must not overlap the inputs.
 *
 * stlt_perturb_curve: logits (S,B,K), row s*B+b at logits + (s*B+b)*ld, ld >= K.  The target class of clip b is target[b] (int64), or with
 * target == NULL the arg-max of its step-0 row (first maximum on ties: stlt_eval_topk's rule), which is written to target_out (B,) — required
 * then, optional (a copy of target) otherwise.  prob (S,B): activation STLT_PERTURB_SOFTMAX — exp(x_t - max) / sum_j exp(x_j - max);
 * STLT_PERTURB_SIGMOID — 1 / (1 + exp(-x_t)); evaluated in float64 and rounded to fp32 once (one value per row is kept).  hit (S,B) uint8: softmax — 1 when no class beats the target (a larger logit, or an equal logit
 * at a lower index: the prediction EvaluatorSomething.process counts, evaluation.py:21-34); sigmoid — 1 when x_t > 0.  A target outside
 * [0, K) gives prob 0 and hit 0.  One wave per row. */
#define STLT_PERTURB_OBJECT 0
#define STLT_PERTURB_FRAME 1
#define STLT_PERTURB_SOFTMAX 0
#define STLT_PERTURB_SIGMOID 1
int64_t stlt_perturb_max_items(void);
int stlt_perturb_rank(const float* scores, const uint8_t* kpm_boxes, const int64_t* lengths, int64_t B, int64_t T, int64_t N, int unit, int descending,
                      int32_t* rank, int32_t* n_candidates, stlt_stream_t stream);
int stlt_perturb_apply(const stlt_inputs* in, const int32_t* rank, const int32_t* n_candidates, int unit, int64_t steps, int64_t s0, int64_t s1,
                       int64_t empty_frame_type, int64_t* categories, float* boxes, float* scores, uint8_t* kpm_boxes, int64_t* frame_types,
                       uint8_t* kpm_frames, int64_t* lengths, int32_t* removed, stlt_stream_t stream);
int stlt_perturb_curve(const float* logits, int64_t ld, const int64_t* target, int activation, int64_t S, int64_t B, int64_t K, float* prob, uint8_t* hit,
                       int64_t* target_out, stlt_stream_t stream);

/* ---- the perturbation test on the appearance side: video cells and feature columns (csrc/perturb.hip) ----
 * The reference's appearance encoder takes no key-padding mask (src/modelling/models.py:269, self.transformer(src=features)), so an appearance
 * token is deleted at the input.  The unit is the CELL: x (B,Cch,T,H,W) float32 contiguous is cut into blocks of (ct,ch,cw) along (T,H,W),
 * ragged last blocks included: the grid is Gt = ceil(T/ct), Gh = ceil(H/ch), Gw = ceil(W/cw), C = Gt*Gh*Gw, cell c = (gt*Gh + gh)*Gw + gw
 * covers frames [ct gt, min(ct gt+ct, T)), rows [ch gh, min(ch gh+ch, H)), columns [cw gw, min(cw gw+cw, W)) of every channel.  For
 * video_frames (B,3,T,H,W) and the R3D-50 trunk the cell is (16,32,32): the trunk's total stride (stem (1,2,2), max-pool 2, three stride-2
 * stages, each rounding the extent up), so that cell c is the stride block — not the receptive field — of appearance token 1 + c
 * (features.flatten(2), models.py:260; token 0 is the CLS token, models.py:262-264, and never a candidate).  For precomputed
 * appearance_features (B,Cf,Gt,Gh,Gw) the cell is (1,1,1): the feature column itself.  The three calls share the contract of the three above:
 * stream-ordered, no allocation, no read-back, capturable; STLT_EINVAL with a message and no launch on a bad extent or a NULL required
 * pointer; alignment of the element type only (16-byte accesses are chosen by the pointers' alignment, see below).  A clip holds fewer than
 * 2^31 elements and at most stlt_perturb_max_items() cells.
 *
 * stlt_perturb_rank_cells: scores (B,C) -> rank (B,C) int32, the position of every cell in the removal order (0 = removed first), and
 * n_candidates (B,) int32 = C: every cell is a candidate.  The order is stlt_perturb_rank's, by the same LDS sort: floats compared with
 * -0 == +0, ties to the lower flat index in both orders, NaN removed last in both orders.  C <= stlt_perturb_max_items(), else STLT_EINVAL.
 *
 * stlt_perturb_apply_cells: for every step s in [s0, s1], 0 <= s0 <= s1 <= steps, steps >= 1, s1-s0+1 <= 256: x with the cells of
 * 0 <= rank < k set to `fill`, k = floor(s * n_candidates[b] / steps) (64-bit product); every other element is copied bit for bit.  fill 0.0
 * is mid-grey after the reference's Normalize(0.5, 0.5) (src/modelling/datasets.py:151).  out ((s1-s0+1)*B, Cch,T,H,W) is step-major like
 * stlt_perturb_apply's: clip (s-s0)*B + b is clip b at step s.  removed ((s1-s0+1), B) int32, optional (NULL): k per step and clip.  rank
 * (B,C) with C the grid's cell count and n_candidates are trusted, not checked: other values blank other cells, inside the extents all the
 * same.  Every source element is read once and written s1-s0+1 times.  Lane accesses are 16 bytes wide when W % 4 == 0, cw % 4 == 0 and x and
 * out are 16-byte aligned, one float wide otherwise: the same bits either way.  out must not overlap x.
 *
 * stlt_cell_pool_abs: out (B,C)[b,c] = the sum of |g| over cell c and all channels of g (B,Cch,T,H,W): video_frames_grad or
 * appearance_features_grad as a per-cell saliency map, as the layout side sums |boxes_grad| over the four coordinates.  The summation
 * order is fixed (no atomics): two launches give the same bits; the error is that of a tree sum of non-negative fp32 terms. */
int stlt_perturb_rank_cells(const float* scores, int64_t B, int64_t C, int descending, int32_t* rank, int32_t* n_candidates, stlt_stream_t stream);
int stlt_perturb_apply_cells(const float* x, int64_t B, int64_t Cch, int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, const int32_t* rank,
                             const int32_t* n_candidates, int64_t steps, int64_t s0, int64_t s1, float fill, float* out, int32_t* removed, stlt_stream_t stream);
int stlt_cell_pool_abs(const float* g, int64_t B, int64_t Cch, int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, float* out, stlt_stream_t stream);
/* stlt_cell_pool_sum: the signed twin of stlt_cell_pool_abs — out (B,C)[b,c] = the sum of g itself over cell c and all channels: a signed
 * attribution map (stlt_ig_reduce's attr) per cell.  The same kernel, extents, refusals and summation order; the error is that of a tree
 * sum of fp32 terms of both signs (bounded by the sum of their magnitudes, not by the result). */
int stlt_cell_pool_sum(const float* g, int64_t B, int64_t Cch, int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, float* out, stlt_stream_t stream);

/* ---- integrated gradients (csrc/integrated_gradients.hip) ----
 * Sundararajan, Taly, Yan 2017: attr = (x - x0) * integral over alpha in [0,1] of dF/dx at x0 + alpha (x - x0), F the seeded logit, x0 a
 * baseline; the attributions sum to F(x) - F(x0) (completeness).  The integral is the trapezoid rule on S = steps + 1 points, steps >= 1:
 * alpha_s = s / steps, w_s = 1 / steps for 0 < s < steps and 1 / (2 steps) for s = 0 and s = steps (the weights sum to 1; both endpoints
 * are on the path, so F(x) and F(x0) come out of the same passes).  The gradients are the existing input-only sweeps'; these entry points
 * build the path, accumulate the quadrature and reduce the completeness gap.  They share one contract: stream-ordered, no allocation, no
 * synchronisation, no read-back, capturable; STLT_EINVAL with a message and no launch on a NULL required pointer, steps < 1 (or >= 2^23),
 * s0 < 0, s0 > s1, s1 > steps, more than STLT_IG_MAX_STEPS steps in one call, or a tensor of 2^31 elements or more; pointers need the
 * alignment of their element type only.
 *
 * The fp32 arithmetic, exactly (fadd / fsub / fmul / fdiv: the IEEE operation rounded to nearest even, never contracted into an FMA — a
 * numpy float32 restatement reproduces every bit):
 *   alpha_s = fdiv((float)s, (float)steps)            w_s = fdiv(1, (float)steps), or fdiv(1, (float)(2 steps)) at s = 0 and s = steps
 *   point_s = fadd(x0, fmul(alpha_s, fsub(x, x0)))    for 0 < s < steps; step 0 is x0's bits and step `steps` is x's bits, not computed
 *   acc     = fadd(acc, fmul(w_s, g_s))               for s = s0, s0+1, ..., s1 in this order, starting from +0 (STLT_IG_BEGIN) or from acc
 *   attr    = fmul(fsub(x, x0), acc)
 * A NULL baseline stands for x0 = +0 (stlt_ig_path) or x0 = fill (the dense calls) in the same formulas.
 *
 * stlt_ig_path: steps s0 .. s1 of the layout batch `in` (stlt_inputs: B, T, N and the seven tensors; scores may be NULL; the row counts are
 * not read), step-major like stlt_perturb_apply: clip (s-s0)*B + b is clip b at step s.  boxes (B,T,N,4) and scores (B,T,N) go to point_s
 * with the baselines boxes0 / scores0 (same shapes, or NULL: zeros); categories, both masks, frame_types and lengths are copied bit for bit.
 * One launch: every input element is read once, every step is written from registers.  Reads B*T*N slots of `in` and of the baselines,
 * writes (s1-s0+1)*B*T*N slots of each output.  The outputs must not overlap the inputs.
 *
 * stlt_ig_path_dense: the same for one dense float32 tensor x of n elements per clip (video_frames (B,3,T,H,W), appearance_features, ...):
 * out ((s1-s0+1)*B, n) step-major.  x0 (B,n), or NULL: every baseline element is `fill`.  Accesses are 16 bytes wide on the aligned body,
 * with a scalar head and tail, when x, x0 and out have the same address modulo 16 and either one step is written or B*n % 4 == 0; one float
 * wide otherwise: the same bits either way.  The grid is sized for the chip's 256 CUs, whatever the host.  Reads B*n, writes (s1-s0+1)*B*n.
 *
 * stlt_ig_reduce: g ((s1-s0+1)*B, n) — the gradients at the path points of steps s0 .. s1, step-major — is added into acc (B,n) in place,
 * one element per lane, ascending s, no atomics.  flags: STLT_IG_BEGIN — acc starts from +0 and is not read (the first call of a sum);
 * STLT_IG_FINISH — after the last step, attr (B,n) = (x - x0) * acc is written (x required; x0 (B,n), or NULL: `fill`).  The steps of a sum
 * may be split over several calls in ascending order: (BEGIN, s0..k) then (k+1..s1, FINISH) gives the bits of (BEGIN | FINISH, s0..s1).
 * grouped (B, n/group), optional with FINISH, 1 <= group <= 64 dividing n: the sum of each run of `group` consecutive attributions, added
 * left to right, then extra (B, n/group) when given.  For the layout: scores first (attr_scores), then boxes with group 4, extra =
 * attr_scores: grouped is object_attribution (B,T,N) = (((a_x1 + a_y1) + a_x2) + a_y2) + a_score.  acc, attr and grouped overlap neither g nor each other.
 *
 * stlt_ig_delta: delta (B,)[b] = the sum of up to three attribution tensors of clip b (a_i (B,n_i); n_i = 0: absent, a_i not read) minus
 * sum_k seed[b,k] * (logits_x[b,k] - logits_x0[b,k]) ((B,K) each): the completeness gap, 0 for an exact integral.  Two stages over a fixed
 * partition: stage 1 writes one fp32 partial per STLT_IG_DELTA_CHUNK consecutive elements of one tensor of one clip (lane t of 256 adds
 * elements t, t+256, ... in order, then the wave, then the four waves) into scratch — stlt_ig_delta_scratch_bytes(B, n0, n1, n2) bytes,
 * 4-byte aligned; stage 2, one workgroup per clip, adds the clip's partials and the K logit terms in fp64 and rounds once.  The chunk is a
 * compile-time constant, so the bits do not depend on the grid: max_blocks (0: the default, sized for 256 CUs) caps stage 1's grid and
 * changes nothing else.  One clip of 3*16*112*112 elements is 147 chunks.  Error against the exact sum of the fp32 attributions: below
 * 2^-23 * (number of addends) * sum|a|. */
#define STLT_IG_MAX_STEPS 256
#define STLT_IG_DELTA_CHUNK 4096
#define STLT_IG_BEGIN 1
#define STLT_IG_FINISH 2
int stlt_ig_path(const stlt_inputs* in, const float* boxes0, const float* scores0, int64_t steps, int64_t s0, int64_t s1, int64_t* categories, float* boxes,
                 float* scores, uint8_t* kpm_boxes, int64_t* frame_types, uint8_t* kpm_frames, int64_t* lengths, stlt_stream_t stream);
int stlt_ig_path_dense(const float* x, const float* x0, float fill, int64_t B, int64_t n, int64_t steps, int64_t s0, int64_t s1, float* out, stlt_stream_t stream);
int stlt_ig_reduce(const float* g, int64_t B, int64_t n, int64_t steps, int64_t s0, int64_t s1, int flags, float* acc, const float* x, const float* x0, float fill,
                   float* attr, int64_t group, const float* extra, float* grouped, stlt_stream_t stream);
size_t stlt_ig_delta_scratch_bytes(int64_t B, int64_t n0, int64_t n1, int64_t n2);
int stlt_ig_delta(const float* a0, int64_t n0, const float* a1, int64_t n1, const float* a2, int64_t n2, const float* seed, const float* logits_x,
                  const float* logits_x0, int64_t B, int64_t K, int64_t max_blocks, void* scratch, size_t scratch_bytes, float* delta, stlt_stream_t stream);

/* ---- class activation maps (csrc/gradcam.hip) ----
 * Grad-CAM (Selvaraju et al., ICCV 2017) at a stage of the trunk: with a the stage's activations and g the gradient of one logit with
 * respect to them, alpha[b,c] = mean over the positions p of g, cam[b,p] = relu(sum_c alpha[b,c] a[b,p,c]); HiResCAM (Draelos and Carin,
 * 2020) multiplies element by element instead: cam[b,p] = relu(sum_c g[b,p,c] a[b,p,c]).  P is the number of positions (t h w), layout
 * STLT_CAM_NDHWC: a and g are (B, P, C), as on the trunk's tape and as stlt_r3d_backward_layer writes; STLT_CAM_NCDHW: (B, C, P), as
 * appearance_features and its gradient.  One contract: stream-ordered, no allocation, no synchronisation, no read-back, capturable; no
 * float atomics, every sum owned by one wave or one fixed group of lanes and added in an order that depends on (P, C, layout) alone, so a
 * clip's values are the same bits whatever B is and from run to run; STLT_EINVAL with a message and no launch on a NULL pointer, B < 0,
 * P < 1, C < 1, a tensor of 2^31 elements or more, an unknown layout or a pointer off its element's 4 bytes; B == 0 returns 0.
 *
 * stlt_cam_weights: alpha (B,C)[b,c] = (sum_p g[b,p,c]) / P.  NDHWC: lanes along c — 16-byte loads when C % 4 == 0 and g is 16-byte
 *     aligned, one float per lane otherwise, the same bits —, P cut into chunks of STLT_CAM_CHUNK positions (four accumulators, position p of
 *     a chunk to accumulator p % 4, then (a0 + a1) + (a2 + a3)); more than one chunk: the partials go to scratch (B, chunks, C) and a second
 *     launch adds them in ascending order; then one division by (float)P.  scratch: stlt_cam_scratch_bytes(B, P, C) bytes (pure host
 *     arithmetic; 0 when P <= STLT_CAM_CHUNK or the shape is refused), 16-byte aligned, STLT_EWORKSPACE otherwise; not read for NCDHW.
 *     NCDHW: a wave per (b,c) row, lane l adds elements l, l + 64, ... in order, then the DPP wave sum (csrc/wave_dpp.h).
 *     Error against the exact mean: below P 2^-24 sum_p|g| / P plus the division's rounding.  Reads B P C floats, writes B C.
 * stlt_cam_map: cam (B,P)[b,p] = sum_c w a, w = alpha (B,C) with per_element == 0 (Grad-CAM), w of a's shape and layout with
 *     per_element != 0 (HiResCAM); relu != 0: a result that is not positive is stored as +0.  NDHWC: a wave per position, lane l an fmaf
 *     chain over the channels of the quads l, l + 64, ... in ascending order (16-byte loads under the alignment rule above, the same bits either way), then the DPP wave sum.
 *     NCDHW: a workgroup per 32 positions of a clip, 16 lane groups, group q an fmaf chain over channels q, q + 16, ..., the 16 partials
 *     added in ascending order.  Error below (C + 1) 2^-24 sum_c|w a|.  Reads B P C floats of a (and of w when per_element), writes B P.
 * stlt_cam_upsample: out (B,T,H,W) = the trilinear resize of cam (B,gt,gh,gw) by the rule of torch's
 *     F.interpolate(mode="trilinear", align_corners=False): per axis the source coordinate of output index d is (in / out) (d + 0.5) - 0.5
 *     in fp32, clamped at 0; its floor i0 and i1 = min(i0 + 1, in - 1) are blended with l1 = the fraction and l0 = 1 - l1, w innermost, then
 *     h, then t.  One thread per output element, coalesced stores; extents from 1 to 65536.  Error below (18 max(gt,gh,gw) + 18) 2^-24 max|cam|. */
#define STLT_CAM_NDHWC 0
#define STLT_CAM_NCDHW 1
#define STLT_CAM_CHUNK 32
size_t stlt_cam_scratch_bytes(int64_t B, int64_t P, int64_t C);
int stlt_cam_weights(const float* g, int64_t B, int64_t P, int64_t C, int layout, float* alpha, void* scratch, size_t scratch_bytes, stlt_stream_t stream);
int stlt_cam_map(const float* a, const float* w, int per_element, int64_t B, int64_t P, int64_t C, int layout, int relu, float* cam, stlt_stream_t stream);
int stlt_cam_upsample(const float* cam, int64_t B, int64_t gt, int64_t gh, int64_t gw, int64_t T, int64_t H, int64_t W, float* out, stlt_stream_t stream);

/* ---- per-kernel timing (bench.py roofline leg): hipEvents around every launch of the whole-path calls ---- */
#define STLT_K_EMBED 0
#define STLT_K_GEMM 1
#define STLT_K_ATTN_SPATIAL 2
#define STLT_K_ATTN_TEMPORAL 3
#define STLT_K_ADDLN 4
#define STLT_K_FRAMES 5
#define STLT_K_GATHER 6
#define STLT_K_LN_BWD 7        /* LayerNorm backward (+ its partial-row reductions) */
#define STLT_K_ATTN_BWD 8      /* attention backward */
#define STLT_K_GELU 9          /* stand-alone GELU forward (training tape) / backward */
#define STLT_K_EMBED_BWD 10    /* embedding / frames-embedding backward */
#define STLT_K_OPTIM 11        /* criterion, gradient norm, AdamW */
#define STLT_K_MISC 12         /* row gathers / scatters, column sums, ragged index, the head's small products, relevance rollouts and combine */
#define STLT_K_MHSA_FUSED 13    /* fused in-projection + causal attention core (stlt_mhsa_fused_fwd): temporal tower */
#define STLT_K_MHSA_FUSED_SPATIAL 14  /* the same kernel's non-causal launches (spatial tower) */
#define STLT_K_ATTN_PROBS 15    /* attention probabilities (stlt_attn_probs_fwd, stlt_attn_probs_cross_fwd; one launch per layer of stlt_forward_attention / stlt_caf_forward_attention) and their gradient-weighted form (stlt_attn_grad_probs; one launch per layer of stlt_train_backward_relevance) */
#define STLT_K_CONV_DGRAD_THIN 16  /* the thin-input data gradient (stlt_conv3d_bwd_data_thin; once per stlt_r3d_backward_inputs with dvideo) */
#define STLT_K_COUNT 17
/* The switch is process-wide; the records (and both calls below) belong to the device that is CURRENT when they are made: a
 * process driving several GPUs collects once per device (with that device current) before it switches timing off, or the
 * other devices' records stay queued. */
int stlt_prof_enable(int on);                       /* 1: record events around each launch (serialises nothing, adds events) */
int stlt_prof_collect(double* ms_out, int64_t* launches_out);  /* sync events, accumulate per-kernel ms / launch counts (STLT_K_COUNT entries each), reset */
/* FLOPs (2*M*N*K summed over the launches) of the matrix-core products enqueued on the current device while timing was on,
 * since the last call: what the roofline of a step is priced with, whatever the schedule (forward, elided layers, backward). */
double stlt_prof_take_gemm_flops(void);
/* The same records launch by launch, in launch order (alternative to stlt_prof_collect: either call drains them): duration from the
 * launch's two events, the FLOPs / algorithmic bytes the launcher declared, and the launcher's note — shape, tile, workgroups, rounds,
 * k-steps — for tools/launch_bound.py, which prices every launch of a step against its own bound.  *n_out = records drained (may exceed
 * cap: the first cap are written). */
#define STLT_PROF_NOTE 160
typedef struct { int kid; int kernels; float us; float reserved; double flops, bytes; char note[STLT_PROF_NOTE]; } stlt_prof_launch;  /* kernels: kernel launches inside the record (a stream-K product = 2) */
int stlt_prof_launches(stlt_prof_launch* out, int64_t cap, int64_t* n_out);

/* Diagnostics only (tools/attn_stamps.py, tools/gemm_block_times.py): when non-NULL, stlt_attn_core_fwd runs its
 * s_memtime-stamped build (8 uint64 phase stamps per item) and stlt_linear_fwd records per-workgroup data into dev_buf:
 * 4 uint64 per workgroup (start / end on the 100 MHz clock, XCC id, tile count), then 48 uint64 per workgroup of per-wave
 * phase stamps (STLT_GEMM_STAMP builds), 1024 spare words and 2 uint64 per workgroup of shader-clock start / end — the
 * GEMM writes the first and the last region whenever the buffer is set, so it must hold stlt_debug_buffer_bytes().
 * Pass NULL to restore normal operation. */
int stlt_debug_set_buffer(void* dev_buf);
size_t stlt_debug_buffer_bytes(void);  /* (54 * compute units of the current device + 1024) * 8 */

/* Opt-in "split-bf16" products (csrc/gemm_bf16x3.hip): every f32 operand element is cut into three bf16 pieces and a product is
 * the six piece products of weight >= 2^-24 on v_mfma_f32_16x16x32_bf16, accumulated in f32 — the dropped terms are below the
 * rounding of an f32 multiply.  terms = 6 turns it on, 0 off; the STLT_GEMM_SPLIT_BF16=6 environment variable is the initial
 * value.  What then runs on it: every nn.Linear forward of the entry points above (stlt_linear_fwd, the whole-path forwards,
 * the training forward, the block calls) and the input-gradient products dX = dY·W of stlt_train_backward and the block
 * backwards (through a transposed copy of W in their scratch), when the launch has whole tiles filling at least half of the
 * workgroups (STLT_X3_MIN_FILL, default 0.5), K % 32 == 0 and K >= 64; everything else — the weight-gradient products, small
 * launches — keeps the f32-MFMA kernel.  Not the default: results agree with the f32 kernel's to f32 rounding (error against an
 * fp64 product within eps_f32 * sqrt(K) of the largest output, the bound of one sequential f32 accumulation: equal to the f32
 * kernel's within 15 % on whole-tile launches, up to ~9x it on small ones, whose stream-K form sums K in short ranges) but are not
 * bit-identical to it; an output is finite exactly where the f32 kernel's is, but infinite operands give NaN where the f32 kernel
 * gives +-inf; and bench.py never reports it as `value` (side objects of the JSON line).  Process-wide switch;
 * STLT_EINVAL for other values. */
int stlt_set_gemm_split_bf16(int terms);

#ifdef __cplusplus
}
#endif
#endif /* STLT_HIP_H */
