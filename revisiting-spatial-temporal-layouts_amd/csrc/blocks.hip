// Block-level training entry points: one native forward and one native reverse call per residual block of the fusion
// models (reference src/modelling/models.py:328-431 — SelfAttentionLayer / CrossAttentionLayer / the feed-forward block —
// and the two halves of nn.TransformerEncoderLayer as configured at :46-52, :118-124, :239-246), so that a CAF / CACNF /
// LCF optimisation step is a few dozen calls through the C-ABI instead of a few hundred op-level ones.  Pure orchestration
// of launchers the STLT path already has; the caller owns the tape tensors and the scratch.
//   attention block:  out = LN_eps( x + drop( MHA(x, c, c; kpm, causal, prob-dropout) · Woᵀ + bo ) )      c = x for self-attention
//   feed-forward block: out = LN_eps( x + drop( W2 · drop_inner( act(W1 x + b1) ) + b2 ) )                 act = GELU | ReLU
// Dropout sites: site0 = attention probabilities / inner dropout, site0 + 1 = the dropout in front of the residual.
#include <cstdlib>
#include "ctx.h"

namespace {

// A block backward's device memory comes in two buffers.  `keep` holds what the block's QUEUED weight-gradient products read (their dY
// operands): while a context defers them (stlt_ctx_dw_defer) the caller keeps this buffer — a few rows x d floats — alive until the flush.
// `work` holds everything that is dead when the call returns its launches (stream-K partial tiles, the attention context gradient, reduction
// pools, a transposed weight for the split-bf16 products): one buffer per stream serves every block.
struct BlockScratch {
  // work
  char* lin;        // stlt_linear_bwd's scratch (stream-K partial tiles + column-sum partials)
  size_t lin_bytes;
  float *dctx, *red;
  float* red_pool;  // 4 x red: the call's partial-row reductions are deferred into one batched launch (StltReduceDefer)
  size_t red_floats;
  float* wt;        // 4 d^2 floats: a transposed weight for the opt-in split-bf16 input-gradient products
  size_t wt_floats, work_total;
  // keep
  float *ds, *da, *dq, *dkv, *dh;
  size_t keep_total;
};

enum { BLOCK_ATTN = 0, BLOCK_FFN = 1 };

// rows = the larger of the query-side and key-side row counts
BlockScratch block_scratch(char* keep, char* work, int64_t rows, int64_t d, int kind) {
  BlockScratch b;
  const size_t f = sizeof(float);
  size_t off = 0;
  char* base = work;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off = stlt_align256(off + bytes); return p; };
  b.lin_bytes = stlt_linear_bwd_scratch_bytes(4 * d);
  b.lin = take(b.lin_bytes);
  b.dctx = (float*)take(kind == BLOCK_ATTN ? (size_t)rows * d * f : 0);
  int64_t red = ln_bwd_scratch_floats(d);
  if (512 * 4 * d > red) red = 512 * 4 * d;
  b.red = (float*)take((size_t)red * f);
  b.red_floats = (size_t)red;
  b.red_pool = (float*)take((size_t)red * 4 * f);
  b.wt_floats = (size_t)4 * d * d;
  b.wt = (float*)take(b.wt_floats * f);
  b.work_total = off;
  off = 0;
  base = keep;
  b.ds = (float*)take((size_t)rows * d * f);
  b.da = (float*)take((size_t)rows * d * f);
  b.dq = (float*)take(kind == BLOCK_ATTN ? (size_t)rows * 3 * d * f : 0);
  b.dkv = (float*)take(kind == BLOCK_ATTN ? (size_t)rows * 2 * d * f : 0);
  b.dh = (float*)take(kind == BLOCK_FFN ? (size_t)rows * 4 * d * f : 0);
  b.keep_total = off;
  return b;
}

// The weight-gradient products of a block are collected and run as ONE grouped stream-K launch at the end of the block's
// backward (gemm.hip: launch_weight_grad_group) when every product contracts over a multiple of 32 rows; otherwise product
// by product (MFMA over the 32-row multiple + the strided kernel for the rest: stlt_linear_bwd).
struct DwList {
  StltWeightGradItem it[4];
  int n = 0;
  void add(const float* dy, int64_t n_out, const float* x, int64_t k_in, int64_t rows, float* g_w) {
    if (g_w && rows > 0) it[n++] = StltWeightGradItem{dy, n_out, x, k_in, rows, g_w};
  }
};
// Collector (stlt_ctx_dw_defer): while the call's context has it on, a block's grouped weight-gradient launch is not made at the end of the
// block's backward — its products are queued in the context and stlt_ctx_dw_flush runs the queue as grouped launches of up to 32 products.  A
// block's own group is 2 - 4 products over 2048 / 2112 rows (18 k-steps per workgroup: 0.39 of the MFMA peak, 34 launches + 34 fix-ups per
// CACNF step); 32 products per launch run at the rate of the STLT sweep's 8-layer groups (0.84).  The caller keeps every operand alive until the
// flush.  The queue lives in the CONTEXT the block call names, not in a thread or the process: torch's autograd engine runs the block backwards
// on its own device thread while the trainer switches the collector and flushes it from the thread that called backward() (a thread-local
// collector queued the products on the engine's thread, where nobody ever flushed them: caught by the GPU suite as all-zero weight gradients in
// a later test); two training loops in one process hold two contexts and never see each other's products.
int flush_dw(const DwList& l, const BlockScratch& sc, hipStream_t s) {
  if (l.n == 0) return 0;
  bool group_ok = true;
  for (int i = 0; i < l.n; ++i) group_ok = group_ok && l.it[i].rows % 32 == 0 && l.it[i].rows <= STLT_DW_GROUP_MAX_ROWS;
  if (stlt_ctx* c = group_ok ? stlt_ctx_current() : nullptr) {
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->dw_on && c->dw_n + l.n <= STLT_DW_DEFER_CAP) {
      for (int i = 0; i < l.n; ++i) c->dw[c->dw_n++] = l.it[i];
      return 0;
    }
  }
  if (group_ok) return launch_weight_grad_group(l.it, l.n, s);
  for (int i = 0; i < l.n; ++i)
    TRY(stlt_linear_bwd(l.it[i].x, l.it[i].g_w /* unused: dx is null */, l.it[i].dy, l.it[i].rows, l.it[i].n_out, l.it[i].k_in, nullptr, l.it[i].g_w, nullptr,
                        nullptr, sc.lin, sc.lin_bytes, (stlt_stream_t)s));
  return 0;
}

// dx (M,K) = dy·W (+ add); the weight gradient dw (N,K) += dyᵀ·x is queued on `dws`; db (N) += column sums of dy.
// N (the contraction length of dx) is a multiple of 32 for every Linear of these blocks (d, 2d, 3d, 4d with d = 64 H).
int linear_bwd(const float* x, const float* w, const float* dy, int64_t M, int64_t N, int64_t K, float* dx, const float* add, float* dw,
               float* db, DwList& dws, const BlockScratch& sc, hipStream_t s) {
  if (dx && M > 0) TRY(stlt_input_grad(dy, N, w, N, K, add, K, dx, K, M, sc.wt, sc.wt_floats, s));
  dws.add(dy, N, x, K, M, dw);
  if (db && M > 0) return launch_colsum_acc(dy, N, M, N, db, sc.red, s);
  return 0;
}

}  // namespace

// ---- the training half-blocks (common.h) ----

int stlt_input_grad(const float* dy, int64_t ld_dy, const float* w, int64_t n_out, int64_t k_in, const float* r, int64_t ldr, float* c, int64_t ldc,
                    int64_t rows, float* wt, size_t wt_floats, hipStream_t s) {
  bool taken = false;
  if (wt && (size_t)(n_out * k_in) <= wt_floats) TRY(launch_input_grad_bf16x3(dy, ld_dy, w, n_out, k_in, r, ldr, c, ldc, rows, wt, s, &taken));
  if (!taken) TRY(launch_input_grad_gemm16(dy, ld_dy, w, n_out, k_in, r, ldr, c, ldc, rows, s, &taken));  // under-filled launches (few rows): whole small tiles, W read as it lies
  return taken ? 0 : launch_gemm(0, 1, dy, ld_dy, w, k_in, nullptr, r, ldr, c, ldc, 0, rows, k_in, n_out, 1, STLT_ACT_NONE, s);
}

int stlt_ffn_hidden_bwd(const float* df, const float* lin2_w, const float* u, float* du, int64_t rows, int64_t d, float* g_lin1_b, StltReduceScope& red,
                        StltDrop dr, uint32_t site, const int* drop_rows, float* wt, size_t wt_floats, hipStream_t s) {
  static const bool fused = [] { const char* e = getenv("STLT_FUSE_GELU_BWD"); return e ? atoi(e) != 0 : true; }();
  const int n_part = (int)((rows + 255) / 256 * 16);
  const bool split = wt && (size_t)(4 * d * d) <= wt_floats && stlt_split_bf16_takes(rows, 4 * d, d, d, d);
  if (fused && g_lin1_b && (size_t)(n_part * 4 * d) <= red.red_floats && d % 32 == 0 && !split) {
    float* part = red.chunk();
    const StltGemmEpi epi{dr, site, drop_rows, part};
    bool small = false;  // the temporal tower at the reference's default batch, the fusion models' blocks (~2048 rows): small tiles, same epilogue (gemm16.hip)
    TRY(launch_input_grad_gemm16(df, d, lin2_w, d, 4 * d, u, 4 * d, du, 4 * d, rows, s, &small, 0, &epi));
    if (!small) TRY(launch_gemm(0, 1, df, d, lin2_w, 4 * d, nullptr, u, 4 * d, du, 4 * d, 0, rows, 4 * d, d, 1, STLT_ACT_GELU_BWD, s, &epi));
    return launch_reduce_slabs(part, 4 * d, n_part, g_lin1_b, 4 * d, 1, s);
  }
  TRY(stlt_input_grad(df, d, lin2_w, d, 4 * d, nullptr, 0, du, 4 * d, rows, wt, wt_floats, s));  // dh
  if (g_lin1_b) return launch_gelu_bwd_colsum(du, u, du, rows, 4 * d, g_lin1_b, red.chunk(), s, dr, site, drop_rows);  // du; lin1_b += colsum(du)
  return launch_gelu_bwd(du, u, du, rows * 4 * d, s, dr, site, drop_rows, 4 * d);
}

int stlt_ffn_half_fwd_train(const stlt_ffn_block_params& p, int act, const float* x, float eps, int64_t rows, int64_t d, float* u, float* h, float* f,
                            float* out, StltDrop dr, StltDrop inner, uint32_t site, const int* drop_rows, hipStream_t s) {
  if (act == STLT_ACT_GELU) {
    TRY(launch_linear_gelu_keep(x, d, p.lin1_w, p.lin1_b, u, h, rows, 4 * d, d, inner, site, drop_rows, s));
  } else {
    TRY(launch_linear(x, d, p.lin1_w, p.lin1_b, h, 4 * d, rows, 4 * d, d, STLT_ACT_RELU, s));
    if (inner.thr) TRY(launch_dropout(h, h, rows * 4 * d, inner, site, s));
  }
  TRY(launch_linear(h, 4 * d, p.lin2_w, p.lin2_b, f, d, rows, d, 4 * d, STLT_ACT_NONE, s));
  return launch_add_layernorm(f, d, x, d, p.ln_w, p.ln_b, eps, rows, d, out, d, s, dr, site + 1, drop_rows);
}

int stlt_ffn_half_bwd_train(const stlt_ffn_block_params& p, const stlt_ffn_block_params& g, int act, const float* dy, const float* x, const float* u,
                            const float* h, const float* f, float eps, int64_t rows, int64_t d, StltDrop dr, StltDrop inner, uint32_t site,
                            const int* drop_rows, const StltHalfBwd& b, hipStream_t s) {
  float* df = b.branch(dr);
  TRY(launch_ln_bwd(dy, d, x, d, f, d, p.ln_w, eps, rows, d, b.ds, d, stlt_grad(g.ln_w), stlt_grad(g.ln_b), b.red->chunk(), s, dr, site + 1, b.dbr, 0,
                    stlt_grad(g.lin2_b), drop_rows));                                                     // ds, df; lin2_b += colsum(df)
  if (act == STLT_ACT_GELU) {
    TRY(stlt_ffn_hidden_bwd(df, p.lin2_w, u, b.dh, rows, d, stlt_grad(g.lin1_b), *b.red, inner, site, drop_rows, b.wt, b.wt_floats, s));
  } else {
    TRY(stlt_input_grad(df, d, p.lin2_w, d, 4 * d, nullptr, 0, b.dh, 4 * d, rows, b.wt, b.wt_floats, s));  // dh = df·W2
    if (inner.thr) TRY(launch_dropout(b.dh, b.dh, rows * 4 * d, inner, site, s));
    TRY(stlt_relu_bwd(b.dh, h, b.dh, rows * 4 * d, (stlt_stream_t)s));  // h > 0 <=> pre-activation > 0 and kept
    if (g.lin1_b) TRY(launch_colsum_acc(b.dh, 4 * d, rows, 4 * d, stlt_grad(g.lin1_b), b.red->chunk(), s));
  }
  return stlt_input_grad(b.dh, 4 * d, p.lin1_w, 4 * d, d, b.ds, d, b.dx, d, rows, b.wt, b.wt_floats, s);  // dx = du·W1 + ds
}

int stlt_attn_half_fwd_train(const stlt_attn_block_params& p, const float* ctx, const float* x, float eps, int64_t rows, int64_t d, float* a, float* out,
                             StltDrop dr, uint32_t site, const int* drop_rows, hipStream_t s) {
  TRY(launch_linear(ctx, d, p.out_proj_w, p.out_proj_b, a, d, rows, d, d, STLT_ACT_NONE, s));
  return launch_add_layernorm(a, d, x, d, p.ln_w, p.ln_b, eps, rows, d, out, d, s, dr, site, drop_rows);
}

int stlt_attn_half_bwd_train(const stlt_attn_block_params& p, const stlt_attn_block_params& g, const float* dy, const float* x, const float* a, float eps,
                             int64_t rows, int64_t d, StltDrop dr, uint32_t site, const int* drop_rows, const StltHalfBwd& b, hipStream_t s) {
  TRY(launch_ln_bwd(dy, d, x, d, a, d, p.ln_w, eps, rows, d, b.ds, d, stlt_grad(g.ln_w), stlt_grad(g.ln_b), b.red->chunk(), s, dr, site, b.dbr, 0,
                    stlt_grad(g.out_proj_b), drop_rows));                                                 // ds, da; out_proj_b += colsum(da)
  return stlt_input_grad(b.branch(dr), d, p.out_proj_w, d, d, nullptr, 0, b.dx, d, rows, b.wt, b.wt_floats, s);  // dctx = da·Wo
}

// the reverse call of an attention block behind stlt_attn_block_bwd_train (abar == NULL: its launches and nothing else) and
// stlt_attn_block_bwd_relevance (abar: one more launch, the block's gradient-weighted map, right before the attention backward)
static int attn_block_bwd(const char* fn, const stlt_attn_block_params* p, const stlt_attn_block_params* g, int64_t d, int64_t H, float eps, const float* x,
                          int64_t Lq, const float* c, int64_t Lk, const uint8_t* kpm, int causal, int64_t S, float drop_p, uint64_t seed, uint32_t site0,
                          const float* q, const float* kv, const float* ctx, const float* a, const float* dy, float* dx, float* dc, float* abar,
                          stlt_ctx* tctx, void* keep, size_t keep_bytes, void* work, size_t work_bytes, stlt_stream_t stream) {
  if (!p || !g || !x || !kpm || !q || !ctx || !a || !dy || !dx || !keep || !work || (c && !kv)) return stlt_set_error(STLT_EINVAL, "%s: null argument", fn);
  if (!stlt_heads_ok(d, H)) return stlt_set_error(STLT_EINVAL, "%s: need d %% H == 0, a head dim of at most 256 and d %% 4 == 0", fn);
  if (S < 0 || Lq <= 0 || Lk <= 0 || S > (int64_t)0x7fffffff / (Lq > Lk ? Lq : Lk)) return stlt_set_error(STLT_EINVAL, "%s: bad shape (S %lld, Lq %lld, Lk %lld)", fn, (long long)S, (long long)Lq, (long long)Lk);
  if (S == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int64_t Mq = S * Lq, Mk = S * Lk;
  const BlockScratch sc = block_scratch((char*)keep, (char*)work, Mq > Mk ? Mq : Mk, d, BLOCK_ATTN);
  if (keep_bytes < sc.keep_total) return stlt_set_error(STLT_EWORKSPACE, "%s: keep buffer %zu B < required %zu B", fn, keep_bytes, sc.keep_total);
  if (work_bytes < sc.work_total) return stlt_set_error(STLT_EWORKSPACE, "%s: work buffer %zu B < required %zu B", fn, work_bytes, sc.work_total);
  StltCtxScope scope(tctx, s);
  if (scope.error()) return scope.error();
  const StltDrop dr = stlt_drop_make(drop_p, seed);
  StltGemmScratch lend(sc.lin, STLT_GEMM_SCRATCH_BYTES);
  StltReduceScope red(sc.red_pool, sc.red_floats * 4, sc.red, sc.red_floats, s);
  // out = LN(x + drop(a)), a = ctx·Woᵀ + bo: ds = residual-path gradient, da = gradient wrt a (= ds without dropout); dctx = da·Wo
  const StltHalfBwd hb{sc.ds, sc.da, nullptr, sc.dctx, &red, sc.wt, sc.wt_floats};
  TRY(stlt_attn_half_bwd_train(*p, *g, dy, x, a, eps, Mq, d, dr, site0 + 1, nullptr, hb, s));
  DwList dws;
  dws.add(hb.branch(dr), d, ctx, d, Mq, stlt_grad(g->out_proj_w));
  // relevance: the block's gradient-weighted attention map from what lies in memory right here — the tape's Q and K/V, and dctx
  if (abar && !c) TRY(launch_attn_grad_probs(q, sc.dctx, kpm, causal, S, Lq, H, d / H, abar, s));
  if (abar && c) TRY(launch_attn_grad_probs_cross(q, d, kv, kv + d, 2 * d, sc.dctx, kpm, causal, S, Lq, Lk, H, d / H, abar, s));
  if (!c) {
    // packed self-attention: dqkv (Mq, 3d); in_proj_b += its column sums (accumulated by the attention backward)
    TRY(launch_attn_bwd(q, sc.dctx, kpm, causal, S, Lq, H, d / H, sc.dq, s, dr, site0, stlt_grad(g->in_proj_b), red.chunk()));
    TRY(linear_bwd(x, p->in_proj_w, sc.dq, Mq, 3 * d, d, dx, sc.ds, stlt_grad(g->in_proj_w), nullptr, dws, sc, s));  // dx = dqkv·Win + ds
  } else {
    TRY(stlt_attn_bwd(q, d, kv, kv + d, 2 * d, sc.dctx, kpm, causal, S, Lq, Lk, H, d / H, drop_p, seed, site0, sc.dq, d, sc.dkv, sc.dkv + d, 2 * d, stream));
    TRY(linear_bwd(x, p->in_proj_w, sc.dq, Mq, d, d, dx, sc.ds, stlt_grad(g->in_proj_w), stlt_grad(g->in_proj_b), dws, sc, s));  // dx = dq·Wq + ds
    TRY(linear_bwd(c, p->in_proj_w + d * d, sc.dkv, Mk, 2 * d, d, dc, nullptr, g->in_proj_w ? stlt_grad(g->in_proj_w) + d * d : nullptr,
                   g->in_proj_b ? stlt_grad(g->in_proj_b) + d : nullptr, dws, sc, s));
  }
  TRY(red.flush());
  return flush_dw(dws, sc, s);
}

extern "C" {

int stlt_ctx_dw_defer(stlt_ctx* c, int mode) {
  if (!stlt_ctx_valid(c)) return stlt_set_error(STLT_EINVAL, "stlt_ctx_dw_defer: not a live context handle");
  std::lock_guard<std::mutex> lk(c->mu);
  if (mode == 1) { c->dw_on = true; return 0; }
  if (mode == 0) { c->dw_on = false; return 0; }
  if (mode == -1) { c->dw_on = false; c->dw_n = 0; return 0; }
  return stlt_set_error(STLT_EINVAL, "stlt_ctx_dw_defer: mode 1 (collect), 0 (stop collecting; queued products stay) or -1 (stop and discard)");
}
int stlt_ctx_dw_pending(stlt_ctx* c) {
  if (!stlt_ctx_valid(c)) return -1;
  std::lock_guard<std::mutex> lk(c->mu);
  return c->dw_n;
}
int stlt_ctx_dw_flush(stlt_ctx* c, void* gemm_scratch, size_t gemm_scratch_bytes, stlt_stream_t stream) {
  if (!stlt_ctx_valid(c)) return stlt_set_error(STLT_EINVAL, "stlt_ctx_dw_flush: not a live context handle");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->dw_n == 0) return 0;
  if (!gemm_scratch || gemm_scratch_bytes < STLT_GEMM_SCRATCH_BYTES) return stlt_set_error(STLT_EWORKSPACE, "stlt_ctx_dw_flush: stlt_gemm_scratch_bytes() of scratch are required");
  StltGemmScratch lend(gemm_scratch, STLT_GEMM_SCRATCH_BYTES);
  hipStream_t s = (hipStream_t)stream;
  int rc = 0, i0 = 0;
  while (i0 < c->dw_n && rc == 0) {
    int i1 = i0;
    for (; i1 < c->dw_n && i1 - i0 < STLT_GEMM_GROUP_MAX; ++i1) {
      const float* lo = c->dw[i1].g_w;
      const float* hi = lo + c->dw[i1].n_out * c->dw[i1].k_in;
      bool clash = false;  // two products into overlapping gradient ranges (a weight shared by two blocks) never share a launch
      for (int j = i0; j < i1 && !clash; ++j) {
        const float* lo2 = c->dw[j].g_w;
        const float* hi2 = lo2 + c->dw[j].n_out * c->dw[j].k_in;
        clash = lo < hi2 && lo2 < hi;
      }
      if (clash) break;
    }
    rc = launch_weight_grad_group(c->dw + i0, i1 - i0, s);
    i0 = i1;
  }
  c->dw_n = 0;
  return rc;
}
size_t stlt_block_keep_bytes(int64_t rows, int64_t d, int kind) {
  if (rows <= 0 || d <= 0 || (kind != BLOCK_ATTN && kind != BLOCK_FFN)) return 0;
  return block_scratch(nullptr, nullptr, rows, d, kind).keep_total;
}
size_t stlt_block_work_bytes(int64_t rows, int64_t d) {
  if (rows <= 0 || d <= 0) return 0;
  return block_scratch(nullptr, nullptr, rows, d, BLOCK_ATTN).work_total;  // the attention block's is the larger layout
}

int stlt_attn_block_fwd_train(const stlt_attn_block_params* p, int64_t d, int64_t H, float eps, const float* x, int64_t Lq, const float* c,
                              int64_t Lk, const uint8_t* kpm, int causal, int64_t S, float drop_p, uint64_t seed, uint32_t site0, float* q,
                              float* kv, float* ctx, float* a, float* out, void* gemm_scratch, size_t gemm_scratch_bytes, stlt_stream_t stream) {
  if (!p || !x || !kpm || !q || !ctx || !a || !out || (c && !kv)) return stlt_set_error(STLT_EINVAL, "stlt_attn_block_fwd_train: null argument");
  if (gemm_scratch && gemm_scratch_bytes < STLT_GEMM_SCRATCH_BYTES) return stlt_set_error(STLT_EWORKSPACE, "stlt_attn_block_fwd_train: gemm scratch too small");
  StltGemmScratch lend(gemm_scratch, STLT_GEMM_SCRATCH_BYTES);  // under-filled products run as stream-K when scratch is lent
  if (!stlt_heads_ok(d, H)) return stlt_set_error(STLT_EINVAL, "stlt_attn_block_fwd_train: need d %% H == 0, a head dim of at most 256 and d %% 4 == 0");
  if (!(drop_p >= 0.f && drop_p < 1.f)) return stlt_set_error(STLT_EINVAL, "dropout probability must be in [0,1)");
  if (!c && Lq != Lk) return stlt_set_error(STLT_EINVAL, "stlt_attn_block_fwd_train: self-attention needs Lq == Lk");
  hipStream_t s = (hipStream_t)stream;
  const StltDrop dr = stlt_drop_make(drop_p, seed);
  const int64_t Mq = S * Lq, Mk = S * Lk;
  const int kid = causal ? STLT_K_ATTN_TEMPORAL : STLT_K_ATTN_SPATIAL;
  if (!c) {  // packed q | k | v
    TRY(launch_linear(x, d, p->in_proj_w, p->in_proj_b, q, 3 * d, Mq, 3 * d, d, STLT_ACT_NONE, s));
    TRY(launch_attn(q, kpm, causal, S, Lq, H, d / H, ctx, kid, s, dr, site0));
  } else {   // q from x, k | v from the other modality's tokens (models.py:362-382)
    TRY(launch_linear(x, d, p->in_proj_w, p->in_proj_b, q, d, Mq, d, d, STLT_ACT_NONE, s));
    TRY(launch_linear(c, d, p->in_proj_w + d * d, p->in_proj_b + d, kv, 2 * d, Mk, 2 * d, d, STLT_ACT_NONE, s));
    TRY(launch_attn_general(q, d, kv, kv + d, 2 * d, kpm, causal, S, Lq, Lk, H, d / H, ctx, kid, s, dr, site0));
  }
  return stlt_attn_half_fwd_train(*p, ctx, x, eps, Mq, d, a, out, dr, site0 + 1, nullptr, s);
}

// g: gradient buffers of the block's parameters (same struct; ACCUMULATED into; null members are skipped).
// dx (S*Lq, d) = gradient wrt x; dc (S*Lk, d) = gradient wrt the context tokens (cross-attention only, may be null).
int stlt_attn_block_bwd_train(const stlt_attn_block_params* p, const stlt_attn_block_params* g, int64_t d, int64_t H, float eps, const float* x,
                              int64_t Lq, const float* c, int64_t Lk, const uint8_t* kpm, int causal, int64_t S, float drop_p, uint64_t seed,
                              uint32_t site0, const float* q, const float* kv, const float* ctx, const float* a, const float* dy, float* dx,
                              float* dc, stlt_ctx* tctx, void* keep, size_t keep_bytes, void* work, size_t work_bytes, stlt_stream_t stream) {
  return attn_block_bwd("stlt_attn_block_bwd_train", p, g, d, H, eps, x, Lq, c, Lk, kpm, causal, S, drop_p, seed, site0, q, kv, ctx, a, dy, dx, dc, nullptr, tctx, keep,
                        keep_bytes, work, work_bytes, stream);
}

// The input-only reverse call of an attention block (every parameter frozen, dropout off, no context) that also writes the block's
// gradient-weighted attention map: dx and dc are the bits stlt_attn_block_bwd_train gives with an all-NULL gradient table and drop_p == 0.
int stlt_attn_block_bwd_relevance(const stlt_attn_block_params* p, int64_t d, int64_t H, float eps, const float* x, int64_t Lq, const float* c, int64_t Lk,
                                  const uint8_t* kpm, int causal, int64_t S, const float* q, const float* kv, const float* ctx, const float* a, const float* dy,
                                  float* dx, float* dc, float* abar, void* keep, size_t keep_bytes, void* work, size_t work_bytes, stlt_stream_t stream) {
  static const stlt_attn_block_params no_grads = {};
  if (!abar) return stlt_set_error(STLT_EINVAL, "stlt_attn_block_bwd_relevance: null argument (abar)");
  if ((uintptr_t)abar & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_block_bwd_relevance: abar must be 4-byte aligned");
  if (((uintptr_t)q | (uintptr_t)kv) & 15) return stlt_set_error(STLT_EINVAL, "stlt_attn_block_bwd_relevance: q and kv must be 16-byte aligned");  // the map launch's rule, checked before any launch
  if (Lq > 256 || Lk > 256) return stlt_set_error(STLT_EINVAL, "stlt_attn_block_bwd_relevance: sequence lengths %lld / %lld unsupported (1 ... 256)", (long long)Lq, (long long)Lk);
  return attn_block_bwd("stlt_attn_block_bwd_relevance", p, &no_grads, d, H, eps, x, Lq, c, Lk, kpm, causal, S, 0.f, 0, 0, q, kv, ctx, a, dy, dx, dc, abar, nullptr, keep,
                        keep_bytes, work, work_bytes, stream);
}

int stlt_ffn_block_fwd_train(const stlt_ffn_block_params* p, int64_t d, float eps, int act, int inner_dropout, const float* x, int64_t M,
                             float drop_p, uint64_t seed, uint32_t site0, float* u, float* h, float* f, float* out, void* gemm_scratch,
                             size_t gemm_scratch_bytes, stlt_stream_t stream) {
  if (!p || !x || !h || !f || !out || (act == STLT_ACT_GELU && !u)) return stlt_set_error(STLT_EINVAL, "stlt_ffn_block_fwd_train: null argument");
  if (gemm_scratch && gemm_scratch_bytes < STLT_GEMM_SCRATCH_BYTES) return stlt_set_error(STLT_EWORKSPACE, "stlt_ffn_block_fwd_train: gemm scratch too small");
  StltGemmScratch lend(gemm_scratch, STLT_GEMM_SCRATCH_BYTES);
  if (act != STLT_ACT_GELU && act != STLT_ACT_RELU) return stlt_set_error(STLT_EINVAL, "stlt_ffn_block_fwd_train: activation must be GELU or ReLU");
  if (!(drop_p >= 0.f && drop_p < 1.f)) return stlt_set_error(STLT_EINVAL, "dropout probability must be in [0,1)");
  hipStream_t s = (hipStream_t)stream;
  const StltDrop dr = stlt_drop_make(drop_p, seed);
  const StltDrop inner = inner_dropout ? dr : StltDrop{0u, 1.0f, 0ull};
  return stlt_ffn_half_fwd_train(*p, act, x, eps, M, d, u, h, f, out, dr, inner, site0, nullptr, s);
}

int stlt_ffn_block_bwd_train(const stlt_ffn_block_params* p, const stlt_ffn_block_params* g, int64_t d, float eps, int act, int inner_dropout,
                             const float* x, int64_t M, float drop_p, uint64_t seed, uint32_t site0, const float* u, const float* h, const float* f,
                             const float* dy, float* dx, stlt_ctx* tctx, void* keep, size_t keep_bytes, void* work, size_t work_bytes, stlt_stream_t stream) {
  if (!p || !g || !x || !h || !f || !dy || !dx || !keep || !work || (act == STLT_ACT_GELU && !u)) return stlt_set_error(STLT_EINVAL, "stlt_ffn_block_bwd_train: null argument");
  if (M < 0 || M > 0x7fffffff || d <= 0 || d % 4 != 0 || d > 16384) return stlt_set_error(STLT_EINVAL, "stlt_ffn_block_bwd_train: bad shape (M %lld, d %lld)", (long long)M, (long long)d);
  if (M == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const BlockScratch sc = block_scratch((char*)keep, (char*)work, M, d, BLOCK_FFN);
  if (keep_bytes < sc.keep_total) return stlt_set_error(STLT_EWORKSPACE, "stlt_ffn_block_bwd_train: keep buffer %zu B < required %zu B", keep_bytes, sc.keep_total);
  if (work_bytes < sc.work_total) return stlt_set_error(STLT_EWORKSPACE, "stlt_ffn_block_bwd_train: work buffer %zu B < required %zu B", work_bytes, sc.work_total);
  StltCtxScope scope(tctx, s);
  if (scope.error()) return scope.error();
  const StltDrop dr = stlt_drop_make(drop_p, seed);
  const StltDrop inner = inner_dropout ? dr : StltDrop{0u, 1.0f, 0ull};
  StltGemmScratch lend(sc.lin, STLT_GEMM_SCRATCH_BYTES);
  StltReduceScope red(sc.red_pool, sc.red_floats * 4, sc.red, sc.red_floats, s);
  const StltHalfBwd hb{sc.ds, sc.da, sc.dh, dx, &red, sc.wt, sc.wt_floats};
  TRY(stlt_ffn_half_bwd_train(*p, *g, act, dy, x, u, h, f, eps, M, d, dr, inner, site0, nullptr, hb, s));
  DwList dws;
  dws.add(hb.branch(dr), d, h, 4 * d, M, stlt_grad(g->lin2_w));  // lin2_w += dfᵀ·h
  dws.add(sc.dh, 4 * d, x, d, M, stlt_grad(g->lin1_w));          // lin1_w += duᵀ·x
  TRY(red.flush());
  return flush_dw(dws, sc, s);
}

}  // extern "C"
