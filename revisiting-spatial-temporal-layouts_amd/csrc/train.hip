// Training step of the STLT path in native code: the forward that records a tape, and the reverse sweep that
// autograd would run for the reference's `loss.backward()` (src/train.py:125-127).  Both are fixed launch
// sequences on the caller's stream (no allocation, no synchronisation).
//
// Tape (fp32, rows padded to a multiple of 32 and zero beyond the logical row count — the caller allocates it
// zero-filled and the kernels never write the padding, which is what lets dW = dYᵀ·X run with a rounded-up
// contraction length):
//   s_embed (tok,d) | per spatial layer: x, qkv(3d), ctx, a, x1, u(4d), h(4d), f | x_sp_out | s_frames (BT,d)
//   | per temporal layer: same 8 buffers on BT rows | x_tp_out | head: h0, u0, z1, z2 (B rows)
//   layer math:  qkv = x·Winᵀ+b ; ctx = attn(qkv) ; a = ctx·Woᵀ+bo ; x1 = LN1(x+a) ; u = x1·W1ᵀ+b1 ; h = gelu(u) ;
//                f = h·W2ᵀ+b2 ; y = LN2(x1+f)   (y is the next layer's x)
#include <cstdlib>
#include <mutex>
#include "ctx.h"

namespace {

inline int64_t up32(int64_t v) { return (v + 31) / 32 * 32; }

struct LayerTape { float *x, *qkv, *ctx, *a, *x1, *u, *h, *f; };

struct Tape {
  int64_t tokp, btp, bp;
  float* s_embed;
  LayerTape sp[64];
  float* sp_out;
  float* s_frames;
  LayerTape tp[64];
  float* tp_out;
  float *h0, *u0, *z1, *z2;
  float* sk;  // stream-K partial tiles (not part of the record: scratch of the forward's GEMM launches)
  char* ridx;  // STLT_FLAG_SKIP_PADDING: the ragged index built by the forward, read again by the backward
  size_t bytes;
};

// carve the tape; base may be null to just size it
static Tape tape_layout(char* base, int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_sp, int64_t n_tp) {
  Tape t;
  t.tokp = up32(B * T * N); t.btp = up32(B * T); t.bp = up32(B);
  size_t off = 0;
  auto take = [&](int64_t rows, int64_t width) { float* p = base ? (float*)(base + off) : nullptr; off = stlt_align256(off + (size_t)rows * width * sizeof(float)); return p; };
  t.s_embed = take(t.tokp, d);
  auto take_layer = [&](LayerTape& l, int64_t rows) {
    l.x = take(rows, d); l.qkv = take(rows, 3 * d); l.ctx = take(rows, d); l.a = take(rows, d);
    l.x1 = take(rows, d); l.u = take(rows, 4 * d); l.h = take(rows, 4 * d); l.f = take(rows, d);
  };
  for (int64_t l = 0; l < n_sp; ++l) take_layer(t.sp[l], t.tokp);
  t.sp_out = take(t.tokp, d);
  t.s_frames = take(t.btp, d);
  for (int64_t l = 0; l < n_tp; ++l) take_layer(t.tp[l], t.btp);
  t.tp_out = take(t.btp, d);
  t.h0 = take(t.bp, d); t.u0 = take(t.bp, d); t.z1 = take(t.bp, d); t.z2 = take(t.bp, d);
  t.sk = take((int64_t)(STLT_GEMM_SCRATCH_BYTES / sizeof(float)), 1);
  t.ridx = (char*)take((int64_t)((ragged_index_bytes(B, T, N) + 3) / 4), 1);
  t.bytes = off;
  return t;
}

// backward scratch: gradient buffers for the spatial phase (tok rows) and, separately, the temporal phase (BT
// rows) so that each one's row padding stays zero; split-K slabs; reduction scratch.
// The output gradients of a layer's four Linears (df, du, da, dqkv) are the operands of its weight-gradient products, which run on
// a second stream beside the NEXT layer's dX chain: two sets per tower, used by alternate layers (GradBufs).
struct GradBufs { float *B, *D, *E, *Q, *H; };  // (rows,d) x3, (rows,3d), (rows,4d)
constexpr int DW_EXTRA_SETS = 6;            // + the tower's own set + the second set = 8 layers per grouped launch
// One tower's buffers: A carries the gradient down the dX chain, C is chain-only scratch (both (rows,d)), sets[0..n_sets-1] are its operand sets.
// The temporal tower with few rows (<= STLT_DW_GROUP_MAX_ROWS; beyond it the sets are large) has eight, so that the weight gradients of up to
// eight layers run as ONE grouped launch (32 products) instead of one launch per layer.
struct TowerScratch { float *A, *C; GradBufs sets[2 + DW_EXTRA_SETS]; int n_sets; };
struct Scratch {
  TowerScratch sp, tp;              // spatial (tokp rows), temporal (btp rows)
  float* sk2;                       // stream-K partial tiles of the second stream's launches
  float *hA, *hB;                   // head: (bp,d) x2
  float *slabs, *red, *sk;
  size_t slab_floats, bytes;
  float* red_pool;                  // chunks of `red_floats` for the sweep's partial rows while their reductions are deferred (StltReduceDefer)
  size_t red_floats, red_pool_floats;
  StltReduceScope* rs = nullptr;    // the sweep's deferral holder: rs->chunk() is the partial-row scratch of the next producer
};

constexpr int MAX_SPLIT = 32;
constexpr int AB_MAX_ROWS = 256;  // attention backward: longest sequence (backward.hip: 64 in LDS, up to 256 streamed)

static bool dw_side_wanted();
static bool defer_wanted() { static const bool on = [] { const char* e = getenv("STLT_TRAIN_DEFER_REDUCE"); return e ? atoi(e) != 0 : true; }(); return on; }

// The optional parts follow the switches the sweep itself reads, so that callers of stlt_train_scratch_bytes do not pay for what a
// configuration never touches: the spatial tower's second operand set (10 tokp d floats: +7 GB at 1024 clips of cfg2) only while the
// side stream is wanted, the reduction pool (<= 256 MB) only while the partial-row reductions are deferred.  They sit BEHIND the fixed
// part, so toggling a switch between two calls moves no fixed buffer; the size is asked again by every stlt_train_backward caller.
static Scratch scratch_layout(char* base, int64_t B, int64_t T, int64_t N, int64_t d, int64_t C) {
  Scratch s;
  const int64_t tokp = up32(B * T * N), btp = up32(B * T), bp = up32(B);
  size_t off = 0;
  auto take = [&](int64_t floats) { float* p = base ? (float*)(base + off) : nullptr; off = stlt_align256(off + (size_t)floats * sizeof(float)); return p; };
  auto take_set = [&](int64_t rows) { return GradBufs{take(rows * d), take(rows * d), take(rows * d), take(rows * 3 * d), take(rows * 4 * d)}; };
  for (TowerScratch* t : {&s.sp, &s.tp}) {  // A, B, C, D, E, Q, H
    const int64_t rows = t == &s.sp ? tokp : btp;
    GradBufs& g = t->sets[0];
    t->A = take(rows * d); g.B = take(rows * d); t->C = take(rows * d); g.D = take(rows * d); g.E = take(rows * d); g.Q = take(rows * 3 * d); g.H = take(rows * 4 * d);
    t->n_sets = 1;
  }
  s.hA = take(bp * d); s.hB = take(bp * d);
  s.slab_floats = (size_t)MAX_SPLIT * 4 * d * d;
  s.slabs = take((int64_t)s.slab_floats);
  int64_t red = ln_bwd_scratch_floats(d);
  if (512 * 4 * d > red) red = 512 * 4 * d;  // gelu_bwd column-sum partials (512 x 4d); attn_bwd needs 256 x 3d
  if ((tokp + 255) / 256 * 16 * 4 * d > red) red = (tokp + 255) / 256 * 16 * 4 * d;  // fused GELU backward: 16 partial rows per 256-row tile row
  if (16 * (T + 5) * d > red) red = 16 * (T + 5) * d;  // frames-embedding parameter partials
  const int64_t eb = embed_bwd_scratch_floats(B * T * N, C, d);
  if (eb > red) red = eb;
  s.red = take(red);
  s.red_floats = (size_t)red;
  s.sk = take((int64_t)(STLT_GEMM_SCRATCH_BYTES / sizeof(float)));
  s.tp.n_sets = btp <= STLT_DW_GROUP_MAX_ROWS ? 2 + DW_EXTRA_SETS : 2;
  for (int i = 1; i < s.tp.n_sets; ++i) s.tp.sets[i] = take_set(btp);
  // ---- optional parts
  s.red_pool_floats = (size_t)red * 24 < ((size_t)64 << 20) ? (size_t)red * 24 : ((size_t)64 << 20);  // <= 256 MB
  if (s.red_pool_floats < (size_t)red || !defer_wanted()) s.red_pool_floats = 0;  // a chunk would not fit, or no deferral
  s.red_pool = s.red_pool_floats ? take((int64_t)s.red_pool_floats) : nullptr;
  const bool side = dw_side_wanted();  // one stream: a layer's products are flushed before the next layer rewrites the set
  if (side) s.sp.sets[s.sp.n_sets++] = take_set(tokp);
  s.sk2 = side ? take((int64_t)(STLT_GEMM_SCRATCH_BYTES / sizeof(float))) : nullptr;
  s.bytes = off;
  return s;
}

// ---- second stream for the weight-gradient products --------------------------------------------------------------------------
// A layer's four weight gradients are off the dX chain (nothing downstream reads them before the optimiser).  They are enqueued
// on a per-device side stream (lower priority: the chain is the critical path) behind an event the chain records, with their own
// stream-K scratch; the chain waits for them only when it is about to reuse their operand buffers (two layers later) and at the
// end of the call.  The products fill the chip while the chain runs its row-wise kernels, fix-ups and under-filled launches.
// STLT_TRAIN_DW_STREAM=0 keeps everything on the caller's stream (A/B runs); STLT_TRAIN_DW_WG / STLT_TRAIN_DX_WG cap the grids of
// the side products / the chain's dX products (0 = uncapped) so that both persistent kernels can be resident at once.
struct DwSide {
  StltSideDevice* dev = nullptr;  // != nullptr: this sweep holds dev->busy (released by DwSideHold)
  hipStream_t s = nullptr;
  hipEvent_t chain[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  bool pending[2] = {false, false};
  bool on = false;
  float* sk = nullptr;
  int flush_no = 0;
};
static int g_dw_side_wanted = -1;  // -1: not read yet (STLT_TRAIN_DW_STREAM, default on); stlt_set_train_side_stream overrides
static bool dw_side_wanted() {
  if (g_dw_side_wanted < 0) { const char* e = getenv("STLT_TRAIN_DW_STREAM"); g_dw_side_wanted = e ? (atoi(e) != 0) : 1; }
  return g_dw_side_wanted != 0;
}
static int dw_side_wg_cap() { static const int n = [] { const char* e = getenv("STLT_TRAIN_DW_WG"); return e ? atoi(e) : 0; }(); return n; }
static int dx_chain_wg_cap() { static const int n = [] { const char* e = getenv("STLT_TRAIN_DX_WG"); return e ? atoi(e) : 0; }(); return n; }

// The side stream and its events belong to the call's context (ctx.h: one set per context and device, created at the first sweep that wants it,
// destroyed with the context); a call that names no context keeps every launch on the caller's stream.
static DwSide dw_side_open(const Scratch& sc, stlt_ctx* ctx) {
  DwSide sd;
  if (!ctx || !dw_side_wanted() || !sc.sk2) return sd;
  StltSideDevice& dv = ctx->side[stlt_current_device() & (STLT_MAX_DEVICES - 1)];
  dv.busy.lock();  // also serialises the one creation per device, whichever thread's sweep comes first
  sd.dev = &dv;
  if (!dv.tried) {
    dv.tried = true;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = least urgent
    bool ok = hipStreamCreateWithPriority(&dv.s, hipStreamNonBlocking, lo) == hipSuccess;
    for (int i = 0; ok && i < 4; ++i) ok = hipEventCreateWithFlags(&dv.ev[i], hipEventDisableTiming) == hipSuccess;
    dv.ok = ok;
    (void)hipGetLastError();
  }
  if (!dv.ok) return sd;
  sd.s = dv.s;
  sd.chain[0] = dv.ev[0]; sd.chain[1] = dv.ev[1]; sd.done[0] = dv.ev[2]; sd.done[1] = dv.ev[3];
  sd.sk = sc.sk2;
  sd.on = true;
  return sd;
}
// the chain is about to write the operand buffers of set `par`: the side products that still read them must have finished
static int dw_side_wait(DwSide* sd, int par, hipStream_t s) {
  if (sd && sd->on && sd->pending[par]) {
    if (hipError_t e = hipStreamWaitEvent(s, sd->done[par], 0); e != hipSuccess) return stlt_set_error((int)e, "train_backward: %s", hipGetErrorString(e));
    sd->pending[par] = false;
  }
  return 0;
}
static int dw_side_join(DwSide* sd, hipStream_t s) {
  TRY(dw_side_wait(sd, 0, s));
  return dw_side_wait(sd, 1, s);
}
// Owner of a sweep's DwSide: on EVERY exit path of the call (error returns included) the caller's stream is made to wait for the
// side products still in flight — they read caller-owned tape and scratch, which torch's allocator recycles by the caller's stream
// alone, and a captured graph must see the fork joined — and the per-device stream / event set is handed back.
struct DwSideHold {
  DwSide* sd; hipStream_t s;
  DwSideHold(DwSide* x, hipStream_t st) : sd(x), s(st) {}
  ~DwSideHold() {
    (void)dw_side_join(sd, s);
    if (sd->dev) { sd->dev->busy.unlock(); sd->dev = nullptr; }
  }
  DwSideHold(const DwSideHold&) = delete;
  DwSideHold& operator=(const DwSideHold&) = delete;
};

// The weight-gradient launches of one tower.  Layers take the operand-buffer sets in turn; the products of `group_layers` consecutive
// layers are collected and flushed as one grouped launch — on the side stream when it is on (behind an event of the chain), else on the
// caller's stream.  A set is rewritten only after the flush that read it has finished.  With two sets a tower flushes per layer; with the temporal
// tower's eight it collects up to eight layers (32 products) per grouped launch (STLT_TRAIN_DW_GROUP_LAYERS=1: two sets, per layer — A/B runs).
struct DwQueue {
  DwSide* side;
  const GradBufs* sets;  // the tower's (TowerScratch)
  int n_sets, group_layers = 1;
  StltWeightGradItem items[STLT_GEMM_GROUP_MAX];
  int n_items = 0, layers_in_chunk = 0, layer_no = 0;
  int set_flush[2 + DW_EXTRA_SETS];  // parity of the side-stream flush still reading the set, -1 = none
  int chunk_sets[2 + DW_EXTRA_SETS];  // sets of the layers collected since the last flush
  DwQueue(DwSide* sd, const TowerScratch& ts) : side(sd), sets(ts.sets), n_sets(ts.n_sets) {
    static const int group_env = [] { const char* e = getenv("STLT_TRAIN_DW_GROUP_LAYERS"); return e ? atoi(e) : 8; }();
    if (n_sets > 2 && group_env > 1) group_layers = group_env < n_sets ? group_env : n_sets;
    else if (n_sets > 2) n_sets = 2;
    for (int& f : set_flush) f = -1;
  }
};
static int dwq_wait_parity(DwQueue& q, int par, hipStream_t s) {
  TRY(dw_side_wait(q.side, par, s));
  for (int k = 0; k < q.n_sets; ++k) if (q.set_flush[k] == par) q.set_flush[k] = -1;
  return 0;
}
static int dwq_begin_layer(DwQueue& q, hipStream_t s, GradBufs& out, int& set_idx) {
  set_idx = q.layer_no++ % q.n_sets;
  if (q.set_flush[set_idx] >= 0) TRY(dwq_wait_parity(q, q.set_flush[set_idx], s));
  out = q.sets[set_idx];
  return 0;
}

static int n_cu_cached() { return stlt_device_cus(); }

// g_w (n_out, k_in) += dYᵀ·X with dY (Mp, n_out), X (Mp, k_in).  A weight matrix is only 18-72 output tiles, so the
// launch runs as stream-K over the token contraction (every CU gets an equal share of k-steps; the fix-up adds the
// partial tiles to g_w in a fixed order).  Without lent scratch it falls back to explicit split-K slabs.
static int weight_grad(const float* dy, int64_t n_out, const float* x, int64_t k_in, int64_t Mp, float* g_w, const Scratch& sc,
                       hipStream_t s) {
  if (!g_w) return 0;
  if (sc.sk) return launch_gemm(1, 1, dy, n_out, x, k_in, nullptr, g_w, k_in, g_w, k_in, 0, n_out, k_in, Mp, 1, STLT_ACT_NONE, s);
  const int64_t tiles = ((n_out + 255) / 256) * ((k_in + 127) / 128);
  const int64_t steps = Mp / 32;
  int64_t want = (2 * n_cu_cached() + tiles - 1) / tiles;
  if (want > MAX_SPLIT) want = MAX_SPLIT;
  int split = 1;
  for (int64_t c = 1; c <= want; ++c) if (steps % c == 0) split = (int)c;
  TRY(launch_gemm(1, 1, dy, n_out, x, k_in, nullptr, nullptr, 0, sc.slabs, k_in, n_out * k_in, n_out, k_in, Mp, split,
                  STLT_ACT_NONE, s));
  return launch_reduce_slabs(sc.slabs, n_out * k_in, split, g_w, n_out * k_in, 1, s);
}

// The sweep's input-gradient products (common.h: stlt_input_grad): while stream-K scratch is lent the split-K slab buffer is unused and
// takes the transposed weight of the opt-in split-bf16 form.
static int dx_product(const float* dy, int64_t ld_dy, const float* w, int64_t n_out, int64_t k_in, const float* r, int64_t ldr, float* c,
                      int64_t ldc, int64_t rows, const Scratch& sc, hipStream_t s) {
  return stlt_input_grad(dy, ld_dy, w, n_out, k_in, r, ldr, c, ldc, rows, sc.sk ? sc.slabs : nullptr, sc.slab_floats, s);
}

// The weight gradients of a layer as ONE grouped stream-K launch (gemm.hip: launch_weight_grad_group) when stream-K
// scratch is lent, else product by product.  Every CU gets an equal share of the four products' k-steps: one pipeline
// fill, at most two partial tiles per workgroup and one fix-up for the layer instead of four of each.
static int weight_grad_all(const StltWeightGradItem* items, int n, const Scratch& sc, hipStream_t s) {
  static const bool grouped = [] { const char* e = getenv("STLT_GEMM_GROUP_DW"); return e ? atoi(e) != 0 : true; }();  // A/B knob
  // Grouping pays where the products are launch-bound (the temporal tower at 64 clips: 54 k-steps per workgroup for all four,
  // 322 -> 266 us); with long contractions (the spatial tower: 378 k-steps per workgroup) the four separate launches are
  // slightly faster — three interleaved A/B pairs of the 64-clip step: 27.17 ms grouped everywhere, 27.07 ms with this limit
  static const int64_t max_rows = [] { const char* e = getenv("STLT_GEMM_GROUP_DW_MAXROWS"); return e ? (int64_t)atoll(e) : STLT_DW_GROUP_MAX_ROWS; }();
  int64_t rows = 0;
  for (int i = 0; i < n; ++i) if (items[i].rows > rows) rows = items[i].rows;
  if (grouped && rows <= max_rows && sc.sk && stlt_gemm_has_scratch()) return launch_weight_grad_group(items, n, s);
  for (int i = 0; i < n; ++i) TRY(weight_grad(items[i].dy, items[i].n_out, items[i].x, items[i].k_in, items[i].rows, items[i].g_w, sc, s));
  return 0;
}

// launch what the queue has collected: one grouped launch (weight_grad_all groups products of <= 4096 rows) on the side stream behind
// the chain's event, or on the caller's stream
static int dwq_flush(DwQueue& q, const Scratch& sc, hipStream_t s) {
  if (q.n_items == 0) return 0;
  DwSide* side = q.side;
  if (side && side->on) {
    const int par = side->flush_no++ & 1;
    TRY(dwq_wait_parity(q, par, s));  // the events of this parity are re-recorded below: nothing may still be waiting on them
    if (hipError_t e = hipEventRecord(side->chain[par], s); e != hipSuccess) return stlt_set_error((int)e, "train_backward: %s", hipGetErrorString(e));
    if (hipError_t e = hipStreamWaitEvent(side->s, side->chain[par], 0); e != hipSuccess) return stlt_set_error((int)e, "train_backward: %s", hipGetErrorString(e));
    int rc = 0;
    {
      StltGemmScratch lend(side->sk, STLT_GEMM_SCRATCH_BYTES);
      StltGemmWgCap cap(dw_side_wg_cap());
      rc = weight_grad_all(q.items, q.n_items, sc, side->s);
    }
    // also after a failed launch: whatever did get enqueued on the side stream is joined by the call's exit path (DwSideHold)
    if (hipError_t e = hipEventRecord(side->done[par], side->s); e != hipSuccess) return stlt_set_error((int)e, "train_backward: %s", hipGetErrorString(e));
    side->pending[par] = true;
    TRY(rc);
    for (int i = 0; i < q.layers_in_chunk; ++i) q.set_flush[q.chunk_sets[i]] = par;
  } else {
    TRY(weight_grad_all(q.items, q.n_items, sc, s));
  }
  q.n_items = 0;
  q.layers_in_chunk = 0;
  return 0;
}

// the two half-blocks of an encoder layer as the shared training half-blocks take them (common.h)
static stlt_ffn_block_params ffn_half(const stlt_layer_params& l) { return {l.lin1_w, l.lin1_b, l.lin2_w, l.lin2_b, l.norm2_w, l.norm2_b}; }
static stlt_attn_block_params attn_half(const stlt_layer_params& l) { return {l.in_proj_w, l.in_proj_b, l.out_proj_w, l.out_proj_b, l.norm1_w, l.norm1_b}; }

// One tower of a call, as the forward and the reverse sweep both see it (built once per call: plan_rows).
struct Tower {
  int64_t d, H;
  const stlt_layer_params* layers; const LayerTape* tape; int64_t n_layers;
  int64_t M, Mp, S, L;           // rows (the real ones under skip-padding), M rounded up to 32, sequences, longest sequence
  const uint8_t* kpm; int causal, kid;
  bool ragged; AttnBwdRagged rg;  // skip-padding: the segments of the rows (seg_start / seg_end: the forward's too) and their backward groups
  const int* rows; int64_t n;    // the only output rows that are read afterwards: the CLS row of every frame / frame lengths-1 of every clip
  bool tail;                     // the last layer produces just those rows (layer_forward with picked rows, layer_backward_tail)
  uint32_t site0;
  uint32_t site(int64_t l) const { return site0 + (uint32_t)(8 * l); }  // dropout sites of layer l: site, site + 1, site + 2
  const AttnBwdRagged* rgp() const { return ragged ? &rg : nullptr; }
};

// Relevance sink of a tower's reverse sweep (stlt_train_backward_relevance), carried the way LayerOpts carries the probabilities sink through
// the forward towers: layer l's gradient-weighted attention map (attn_grad_probs.hip) goes to abar + l * S*L*L, written from the layer's
// packed QKV on the tape and dctx right before its attention backward.  stop_at_first: the sweep needs nothing below layer 0's map, so the
// layer returns once it is written.  No sink (every other entry point): not one launch more or less.
struct RelSink { float* abar; bool stop_at_first; };
static int relevance_map(const Tower& tw, int64_t l, const float* qkv, const float* dctx, const RelSink& rel, hipStream_t s) {
  return launch_attn_grad_probs(qkv, dctx, tw.kpm, tw.causal, tw.S, tw.L, tw.H, tw.d / tw.H, rel.abar + l * tw.S * tw.L * tw.L, s);
}

// backward of layer l of a tower.  dy: gradient wrt the layer output (M,d) in ts.A; on return ts.A holds the gradient wrt the layer
// input.  The layer takes the queue's next set of operand buffers — bufB / bufD / bufE (M,d), bufQ (M,3d), bufH (M,4d), scratch with zero
// row padding — waiting for the flush that still reads it, if any; ts.C (M,d) is chain-only scratch.
// The four output gradients of the layer's Linears stay alive until the end of the layer, where their weight-gradient products are left with the
// queue: df in bufD / da in bufE (dropout off: df in bufB, the residual-path gradient — StltHalfBwd::branch), du in bufH, dqkv in bufQ.
static int layer_backward(const Tower& tw, int64_t l, const stlt_layer_params* g, const TowerScratch& ts, const Scratch& sc, StltDrop dr,
                          hipStream_t s, DwQueue& q, const RelSink* rel = nullptr) {
  const stlt_layer_params& lp = tw.layers[l];
  const stlt_layer_params gl = g ? *g : stlt_layer_params{};  // null members are skipped
  const LayerTape& t = tw.tape[l];
  const int64_t d = tw.d, M = tw.M;
  const uint32_t site0 = tw.site(l);
  int set_idx = 0;
  GradBufs gb;
  TRY(dwq_begin_layer(q, s, gb, set_idx));
  float *bufA = ts.A, *bufC = ts.C, *bufB = gb.B, *bufD = gb.D, *bufE = gb.E, *bufQ = gb.Q, *bufH = gb.H;
  StltGemmWgCap chain_cap(q.side && q.side->on ? dx_chain_wg_cap() : 0);
  // y = LN2(x1 + drop(f)), f = h·W2ᵀ + b2, h = drop(gelu(u)), u = x1·W1ᵀ + b1: bufB = ds2, df, bufH = du, bufC = dx1 = du·W1 + ds2
  const StltHalfBwd ffn{bufB, bufD, bufH, bufC, sc.rs, sc.sk ? sc.slabs : nullptr, sc.slab_floats};
  TRY(stlt_ffn_half_bwd_train(ffn_half(lp), ffn_half(gl), STLT_ACT_GELU, bufA, t.x1, t.u, t.h, t.f, 1e-5f, M, d, dr, dr, site0 + 2, nullptr, ffn, s));
  // x1 = LN1(x + drop(a)), a = ctx·Woᵀ + bo: ds1 (in bufB when dropout is on: its ds2 is dead by then), da in bufE, bufC = dctx
  const StltHalfBwd att{dr.thr ? bufB : bufE, bufE, nullptr, bufC, sc.rs, ffn.wt, ffn.wt_floats};
  TRY(stlt_attn_half_bwd_train(attn_half(lp), attn_half(gl), bufC, t.x, t.a, 1e-5f, M, d, dr, site0 + 1, nullptr, att, s));
  if (rel) {
    TRY(relevance_map(tw, l, t.qkv, bufC, *rel, s));
    if (rel->stop_at_first && l == 0) return 0;
  }
  // ctx = attention(qkv) with dropout on the probabilities
  TRY(launch_attn_bwd(t.qkv, bufC, tw.kpm, tw.causal, tw.S, tw.L, tw.H, d / tw.H, bufQ, s, dr, site0, stlt_grad(gl.in_proj_b), sc.rs->chunk(), tw.rgp()));  // bufQ = dqkv; in_proj_b += colsum(dqkv)
  // qkv = x·Winᵀ + bin
  TRY(dx_product(bufQ, 3 * d, lp.in_proj_w, 3 * d, d, att.ds, d, bufA, d, M, sc, s));  // bufA = dx = dqkv·Win + ds1
  // the four weight gradients (off the dX chain): one grouped launch
  const StltWeightGradItem items[4] = {{ffn.branch(dr), d, t.h, 4 * d, tw.Mp, stlt_grad(gl.lin2_w)},
                                       {bufH, 4 * d, t.x1, d, tw.Mp, stlt_grad(gl.lin1_w)},
                                       {att.branch(dr), d, t.ctx, d, tw.Mp, stlt_grad(gl.out_proj_w)},
                                       {bufQ, 3 * d, t.x, d, tw.Mp, stlt_grad(gl.in_proj_w)}};
  for (int i = 0; i < 4; ++i) q.items[q.n_items++] = items[i];
  q.chunk_sets[q.layers_in_chunk++] = set_idx;
  if (q.layers_in_chunk >= q.group_layers || q.n_items + 4 > STLT_GEMM_GROUP_MAX) return dwq_flush(q, sc, s);
  return 0;
}

// in-projection + attention core of a training forward: the packed projections stay in the tape (t.qkv) for the reverse sweep.
// Padded layout, sequences of <= 64 tokens: one fused launch (mhsa.hip, TRAIN build: dropout of the probabilities from the
// counter mask, q / k / v written from the accumulators); ragged layout and other shapes: product + attention core.
static int qkv_attention_train(const Tower& tw, const stlt_layer_params& lp, const LayerTape& t, StltDrop dr, uint32_t site0, hipStream_t s) {
  const int64_t d = tw.d, H = tw.H;
  if (!tw.ragged && stlt_fused_mhsa_on(tw.causal) && stlt_mhsa_fused_pays(tw.S, tw.L, H, d, tw.causal) && !stlt_split_bf16_takes(tw.M, 3 * d, d, d, d))
    return launch_mhsa_fused(t.x, lp.in_proj_w, lp.in_proj_b, tw.kpm, tw.S, tw.L, H, d, t.ctx, s, tw.causal, t.qkv, dr, site0);
  TRY(launch_linear(t.x, d, lp.in_proj_w, lp.in_proj_b, t.qkv, 3 * d, tw.M, 3 * d, d, STLT_ACT_NONE, s));
  if (tw.ragged) return launch_attn_ragged(t.qkv, tw.rg.seg_start, tw.rg.seg_end, tw.causal, tw.M, H, d / H, t.ctx, tw.kid, s, dr, site0);
  return launch_attn(t.qkv, tw.kpm, tw.causal, tw.S, tw.L, H, d / H, t.ctx, tw.kid, s, dr, site0);
}

// Layer l of a tower's training forward, output to y.  Every layer but a tail: every row (n = M; t.ctx / t.x are read in place, no gathers).
// The tail (tw.tail): the last layer of a tower when only n of its M output rows are read afterwards (the CLS row of every frame after
// the spatial tower, models.py:79; frame lengths-1 of every clip after the temporal tower, models.py:189-192): the
// in-projection and the attention run on all rows (every row is a key / value), out-proj, norms and FFN on the picked
// rows only.  Tape: x, qkv, ctx hold M rows; a, x1, u, h, f hold n rows; the gathered ctx / x rows are parked in the
// unused upper part of a / x1 (rows n..2n-1, hence the 2n <= M condition of plan_rows) and re-gathered by the
// reverse sweep.  Dropout masks keep the indices of the rows' original positions.
static int layer_forward(const Tower& tw, int64_t l, float* y, StltDrop dr, hipStream_t s) {
  const stlt_layer_params& lp = tw.layers[l];
  const LayerTape& t = tw.tape[l];
  const bool tail = tw.tail && l == tw.n_layers - 1;
  const int* rows = tail ? tw.rows : nullptr;
  const int64_t d = tw.d, n = tail ? tw.n : tw.M;
  const uint32_t site0 = tw.site(l);
  TRY(qkv_attention_train(tw, lp, t, dr, site0, s));
  const float *ctx = t.ctx, *x = t.x;
  if (rows) {
    float* g_ctx = t.a + n * d;
    float* g_x = t.x1 + n * d;
    TRY(launch_gather_rows(t.ctx, d, rows, n, d, g_ctx, s));
    TRY(launch_gather_rows(t.x, d, rows, n, d, g_x, s));
    ctx = g_ctx;
    x = g_x;
  }
  TRY(stlt_attn_half_fwd_train(attn_half(lp), ctx, x, 1e-5f, n, d, t.a, t.x1, dr, site0 + 1, rows, s));
  return stlt_ffn_half_fwd_train(ffn_half(lp), STLT_ACT_GELU, t.x1, 1e-5f, n, d, t.u, t.h, t.f, y, dr, dr, site0 + 2, rows, s);
}

static int zero_rows(float* buf, int64_t width, int64_t r0, int64_t r1, hipStream_t s) {
  if (r1 <= r0) return 0;
  if (hipError_t e = hipMemsetAsync(buf + r0 * width, 0, (size_t)(r1 - r0) * width * sizeof(float), s); e != hipSuccess)
    return stlt_set_error((int)e, "train_backward: memset: %s", hipGetErrorString(e));
  return 0;
}

// Reverse of layer_forward's tail form.  dy: gradient wrt the n output rows; on return ts.A holds the gradient wrt all M
// input rows.  Scratch roles as in layer_backward, on the tower's own set; the gradient-side operands of the weight-gradient products are
// zeroed between n and its round-up to 32 first (those rows belong to other layers' data in the shared buffers).
static int layer_backward_tail(const Tower& tw, int64_t l, const stlt_layer_params* g, const float* dy, const TowerScratch& ts, const Scratch& sc,
                               StltDrop dr, hipStream_t s, const RelSink* rel = nullptr) {
  const stlt_layer_params& lp = tw.layers[l];
  const stlt_layer_params gl = g ? *g : stlt_layer_params{};
  const LayerTape& t = tw.tape[l];
  const int64_t d = tw.d, M = tw.M, n = tw.n, np = up32(n);
  const int* rows = tw.rows;
  const uint32_t site0 = tw.site(l);
  const GradBufs& gb = ts.sets[0];
  float *bufA = ts.A, *bufC = ts.C, *bufB = gb.B, *bufD = gb.D, *bufE = gb.E, *bufQ = gb.Q, *bufH = gb.H;
  for (float* b : {bufB, bufD, bufE}) TRY(zero_rows(b, d, n, np, s));
  TRY(zero_rows(bufH, 4 * d, n, np, s));
  // the feed-forward half on the picked rows: bufB = ds2, df, bufH = du, bufC = dx1 = du·W1 + ds2
  const StltHalfBwd ffn{bufB, bufD, bufH, bufC, sc.rs, sc.sk ? sc.slabs : nullptr, sc.slab_floats};
  TRY(stlt_ffn_half_bwd_train(ffn_half(lp), ffn_half(gl), STLT_ACT_GELU, dy, t.x1, t.u, t.h, t.f, 1e-5f, n, d, dr, dr, site0 + 2, rows, ffn, s));
  // x1 = LN1(x[rows] + drop(a)), a = ctx[rows]·Woᵀ + bo: gather the two inputs again (bufQ is free until the attention backward)
  float* g_x = bufQ;
  float* g_ctx = bufQ + np * d;
  TRY(launch_gather_rows(t.x, d, rows, n, d, g_x, s));
  TRY(launch_gather_rows(t.ctx, d, rows, n, d, g_ctx, s));
  const StltHalfBwd att{dr.thr ? bufB : bufE, bufE, nullptr, bufC, sc.rs, ffn.wt, ffn.wt_floats};  // ds1, da; bufC = dctx of the picked rows
  TRY(stlt_attn_half_bwd_train(attn_half(lp), attn_half(gl), bufC, g_x, t.a, 1e-5f, n, d, dr, site0 + 1, rows, att, s));
  // the weight gradients of the three Linears that ran on the picked rows: one grouped launch, before bufH / bufQ are reused
  const StltWeightGradItem items[3] = {{ffn.branch(dr), d, t.h, 4 * d, np, stlt_grad(gl.lin2_w)},
                                       {bufH, 4 * d, t.x1, d, np, stlt_grad(gl.lin1_w)},
                                       {att.branch(dr), d, g_ctx, d, np, stlt_grad(gl.out_proj_w)}};
  TRY(weight_grad_all(items, 3, sc, s));
  // the other rows' attention outputs were never read: their dctx is zero
  TRY(launch_scatter_rows(bufC, rows, n, d, bufH, M, s));                                           // bufH (as M x d) = dctx
  if (rel) {
    TRY(relevance_map(tw, l, t.qkv, bufH, *rel, s));
    if (rel->stop_at_first && l == 0) return 0;
  }
  TRY(launch_attn_bwd(t.qkv, bufH, tw.kpm, tw.causal, tw.S, tw.L, tw.H, d / tw.H, bufQ, s, dr, site0, stlt_grad(gl.in_proj_b), sc.rs->chunk(), tw.rgp()));  // bufQ = dqkv
  TRY(weight_grad(bufQ, 3 * d, t.x, d, tw.Mp, stlt_grad(gl.in_proj_w), sc, s));
  TRY(launch_scatter_rows(att.ds, rows, n, d, bufC, M, s));                                            // residual path: ds1 on the picked rows only
  TRY(dx_product(bufQ, 3 * d, lp.in_proj_w, 3 * d, d, bufC, d, bufA, d, M, sc, s));  // bufA = dx = dqkv·Win + ds1
  // the 4d-wide view of bufH lost its zero rows past M to the dctx image only below M*d floats: nothing to restore
  return 0;
}

// Reverse of a whole tower: on return ts.A holds the gradient wrt the tower's input rows.  dy: the gradient wrt the tw.n output rows that were
// read (the tail layer takes it as it is, a tower without one scatters it over zeros); nullptr: ts.A already holds the gradient wrt every output row.
// g: the tower's gradient table, or nullptr.  The closing flush launches what a grouping queue still holds (nothing when it flushes per layer).
static int tower_backward(const Tower& tw, const stlt_layer_params* g, const float* dy, const TowerScratch& ts, const Scratch& sc, StltDrop dr,
                          hipStream_t s, DwQueue& q, const RelSink* rel = nullptr) {
  int64_t l = tw.n_layers - 1;
  if (tw.tail) {
    TRY(layer_backward_tail(tw, l, g ? &g[l] : nullptr, dy, ts, sc, dr, s, rel));
    --l;
  } else if (dy) {
    TRY(launch_scatter_rows(dy, tw.rows, tw.n, tw.d, ts.A, tw.Mp, s));
  }
  for (; l >= 0; --l) TRY(layer_backward(tw, l, g ? &g[l] : nullptr, ts, sc, dr, s, q, rel));
  return dwq_flush(q, sc, s);
}

// The weight-gradient products contract over the row count rounded up to 32: the rows of a queue's operand sets between the count and its
// round-up are cleared (at most 31 rows per buffer).
static int clear_operand_padding(const DwQueue& q, const Tower& tw, hipStream_t s) {
  for (int k = 0; k < q.n_sets; ++k) {
    for (float* b : {q.sets[k].B, q.sets[k].D, q.sets[k].E}) TRY(zero_rows(b, tw.d, tw.M, tw.Mp, s));
    TRY(zero_rows(q.sets[k].Q, 3 * tw.d, tw.M, tw.Mp, s));
    TRY(zero_rows(q.sets[k].H, 4 * tw.d, tw.M, tw.Mp, s));
  }
  return 0;
}

static int check_train(const stlt_params* p, const stlt_inputs* in, int flags) {
  const bool need_head = !(flags & STLT_FLAG_TRAIN_BACKBONE);
  if (!p || !in) return stlt_set_error(STLT_EINVAL, "null params/inputs");
  if (!stlt_heads_ok(p->d, p->H))
    return stlt_set_error(STLT_EINVAL, "hidden_size %lld / heads %lld: need hidden_size %% heads == 0, a head dim of at most 256 and hidden_size %% 4 == 0", (long long)p->d, (long long)p->H);
  if (p->n_spatial < 0 || p->n_spatial > 64 || p->n_temporal < 0 || p->n_temporal > 64) return stlt_set_error(STLT_EINVAL, "layer count out of range");
  if (in->B <= 0 || in->T <= 0 || in->N <= 0 || in->T > p->n_positions) return stlt_set_error(STLT_EINVAL, "bad batch shape");
  if (!in->categories || !in->boxes || !in->kpm_boxes || !in->frame_types || !in->kpm_frames || !in->lengths)
    return stlt_set_error(STLT_EINVAL, "null input tensor");
  if (need_head && (!p->fc1_w || !p->fc2_w || p->n_classes <= 0)) return stlt_set_error(STLT_EINVAL, "prediction head missing");
  if (p->n_categories > STLT_TRAIN_MAX_CATEGORIES)  // the embedding-gradient kernel keeps per-category sums in LDS (backward.hip: embed_bwd_kernel)
    return stlt_set_error(STLT_EINVAL, "training supports at most %d object categories (got %lld)", STLT_TRAIN_MAX_CATEGORIES, (long long)p->n_categories);
  if (!need_head && (flags & STLT_FLAG_SKIP_PADDING)) return stlt_set_error(STLT_EINVAL, "STLT_FLAG_TRAIN_BACKBONE excludes STLT_FLAG_SKIP_PADDING");
  return 0;
}

// An input-only sweep (stlt_train_backward_inputs with a table of NULLs: saliency, a frozen model whose layout requires grad) names no
// parameter gradient at all: then there is no weight-gradient product to fork a stream for and no operand row padding to clear.
static bool layer_table_empty(const stlt_layer_params& l) {
  return !l.in_proj_w && !l.in_proj_b && !l.out_proj_w && !l.out_proj_b && !l.lin1_w && !l.lin1_b && !l.lin2_w && !l.lin2_b && !l.norm1_w && !l.norm1_b &&
         !l.norm2_w && !l.norm2_b;
}
static bool grad_table_empty(const stlt_params* p, const stlt_params* g) {
  if (g->cat_emb || g->box_w || g->box_b || g->score_w || g->score_b || g->emb_ln_w || g->emb_ln_b || g->pos_emb || g->type_emb || g->frames_ln_w ||
      g->frames_ln_b || g->fc1_w || g->fc1_b || g->head_ln_w || g->head_ln_b || g->fc2_w || g->fc2_b)
    return false;
  for (int64_t l = 0; g->spatial && l < p->n_spatial; ++l) if (!layer_table_empty(g->spatial[l])) return false;
  for (int64_t l = 0; g->temporal && l < p->n_temporal; ++l) if (!layer_table_empty(g->temporal[l])) return false;
  return true;
}

// What the forward and the reverse sweep of one call must agree on, computed in one place for both: the opened tape, the schedule (padded /
// skip-padding), the row counts, which towers end in a tail layer, and each tower's descriptor with its dropout sites.  Two steps, because the
// argument checks that sit between them come in a fixed order (tests/host_fuzz.hip tallies which one a bad call reports).
struct Plan {
  bool backbone_only, ragged, host_counts = false;  // backbone_only (STLT_FLAG_TRAIN_BACKBONE): no head, `logits` / `dlogits` are the (B*T, d) backbone output / its gradient
  Tape t;
  RaggedIndex ix;  // the ragged index (skip-padding), or the padded layout's picked rows: built by the forward, read again by the backward
  int64_t tok, BT;
  int fpg;         // skip-padding: whole frames per attention-backward group of the spatial tower
  Tower sp, tp;    // (they point into t: a Plan is filled in place and never copied)
};
static int plan_open(Plan& pl, const stlt_params* p, const stlt_inputs* in, const void* tape_mem, size_t tape_bytes, int flags) {
  pl.backbone_only = (flags & STLT_FLAG_TRAIN_BACKBONE) != 0;
  // Padded schedule: every (clip, frame, slot) row, masks applied inside the attention.  Skip-padding: the same launches over the real rows
  // only (ragged.hip): the tape holds those alone (same buffers, fewer rows) and dropout masks are drawn per compacted row.
  pl.ragged = (flags & STLT_FLAG_SKIP_PADDING) != 0;
  pl.t = tape_layout((char*)const_cast<void*>(tape_mem), in->B, in->T, in->N, p->d, p->n_spatial, p->n_temporal);
  if (tape_bytes < pl.t.bytes) return stlt_set_error(STLT_EWORKSPACE, "tape %zu B < required %zu B", tape_bytes, pl.t.bytes);
  if ((uintptr_t)tape_mem & 255) return stlt_set_error(STLT_EINVAL, "tape must be 256-byte aligned");
  pl.ix = ragged_index_carve(pl.t.ridx, in->B, in->T, in->N);
  return 0;
}
// the row counts (skip-padding: the caller's, or read back from the index — the forward, `pad`, has just built it) and what follows from them
static int plan_rows(Plan& pl, const stlt_params* p, const stlt_inputs* in, bool pad, hipStream_t s) {
  const int64_t B = in->B, T = in->T, N = in->N;
  const RaggedIndex& ix = pl.ix;
  pl.tok = B * T * N; pl.BT = B * T;
  if (pl.ragged) TRY(read_ragged_counts(ix, in, pad, pl.tok, pl.BT, &pl.host_counts, s));
  const int64_t tok = pl.tok, BT = pl.BT;
  pl.fpg = N <= 32 ? (int)(32 / N) : 1;
  // the last layer of each tower only has to produce the rows that are read afterwards
  pl.sp = Tower{p->d, p->H, p->spatial, pl.t.sp, p->n_spatial, tok, up32(tok), B * T, N, in->kpm_boxes, 0, STLT_K_ATTN_SPATIAL, pl.ragged,
                AttnBwdRagged{ix.sp_grp_ptr, ix.t_seg_start, ix.t_seg_end, (BT + pl.fpg - 1) / pl.fpg, tok, (int)(pl.fpg * N)},
                ix.f_cls_row, BT, p->n_spatial > 0 && 2 * BT <= tok, 8u};
  pl.tp = Tower{p->d, p->H, p->temporal, pl.t.tp, p->n_temporal, BT, up32(BT), B, T, in->kpm_frames, 1, STLT_K_ATTN_TEMPORAL, pl.ragged,
                AttnBwdRagged{ix.clip_frm_off, ix.f_seg_start, ix.f_seg_end, B, BT, (int)T},
                ix.last_row, B, !pl.backbone_only && p->n_temporal > 0 && 2 * B <= BT, (uint32_t)(8 * (p->n_spatial + 1))};
  return 0;
}

// The end of a relevance sweep: both rollouts, the combine, and what every exit of the sweep does.
static int relevance_finish(const stlt_params* p, const stlt_inputs* in, const stlt_relevance_maps* maps, StltReduceScope& red, hipStream_t s) {
  const int64_t B = in->B, T = in->T, N = in->N;
  TRY(launch_attn_rollout(maps->abar_spatial, p->n_spatial, B * T, N, maps->rollout_spatial, s));
  TRY(launch_attn_rollout(maps->abar_temporal, p->n_temporal, B, T, maps->rollout_temporal, s));
  if (maps->relevance)  // (NULL under STLT_FLAG_TRAIN_BACKBONE: the fusion models read the rollouts out with stlt_relevance_combine_joint)
    TRY(launch_relevance_combine(maps->rollout_temporal, maps->rollout_spatial, in->lengths, B, T, N, maps->relevance, s));
  return red.flush();
}

}  // namespace

extern "C" {

int stlt_set_train_side_stream(int on) { g_dw_side_wanted = on < 0 ? -1 : (on != 0); return 0; }  // < 0: back to STLT_TRAIN_DW_STREAM / the default
int stlt_get_train_side_stream(void) { return dw_side_wanted() ? 1 : 0; }

size_t stlt_train_tape_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_spatial, int64_t n_temporal) {
  if (B <= 0 || T <= 0 || N <= 0 || d <= 0 || n_spatial < 0 || n_spatial > 64 || n_temporal < 0 || n_temporal > 64) return 0;
  return tape_layout(nullptr, B, T, N, d, n_spatial, n_temporal).bytes;
}

size_t stlt_train_scratch_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_categories) {
  if (B <= 0 || T <= 0 || N <= 0 || d <= 0 || n_categories <= 0 || n_categories > STLT_TRAIN_MAX_CATEGORIES) return 0;
  return scratch_layout(nullptr, B, T, N, d, n_categories).bytes;
}

int stlt_train_forward(const stlt_params* p, const stlt_inputs* in, void* tape_mem, size_t tape_bytes, float* logits,
                       float dropout_p, uint64_t dropout_seed, int flags, stlt_stream_t stream) {
  TRY(check_train(p, in, flags));
  if (!logits || !tape_mem) return stlt_set_error(STLT_EINVAL, "stlt_train_forward: null logits/tape");
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = in->B, T = in->T, N = in->N, d = p->d;
  Plan pl;
  TRY(plan_open(pl, p, in, tape_mem, tape_bytes, flags));
  const Tape& t = pl.t; const RaggedIndex& ix = pl.ix; const bool ragged = pl.ragged, backbone_only = pl.backbone_only;
  StltGemmScratch gemm_scratch(t.sk, STLT_GEMM_SCRATCH_BYTES);
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return stlt_set_error(STLT_EINVAL, "dropout probability must be in [0,1)");
  const StltDrop dr = stlt_drop_make(dropout_p, dropout_seed);
  if (ragged) {
    if (N > AB_MAX_ROWS || T > AB_MAX_ROWS)  // the reverse sweep would refuse the tape anyway; head dims other than 64 hold a segment's keys in LDS
      return stlt_set_error(STLT_EINVAL, "skip-padding training supports sequences of at most %d tokens (N=%lld, T=%lld)", AB_MAX_ROWS, (long long)N, (long long)T);
    TRY(launch_ragged_index(in->kpm_boxes, in->kpm_frames, in->lengths, B, T, N, ix, s));
  } else {
    TRY(launch_padded_rows(in->lengths, B, T, N, ix, s));  // rows the tail layers pick: f*N and b*T + lengths-1
  }
  TRY(plan_rows(pl, p, in, true, s));
  const int64_t tok = pl.tok, BT = pl.BT;
  float* x0 = p->n_spatial > 0 ? t.sp[0].x : t.sp_out;
  TRY(launch_embed(in->categories, in->boxes, in->scores, p->cat_emb, p->n_categories, p->box_w, p->box_b, p->score_w,
                   p->score_b, p->emb_ln_w, p->emb_ln_b, p->ln_eps, tok, d, x0, s, t.s_embed, dr, ragged ? ix.t_orig : nullptr));
  for (int64_t l = 0; l < p->n_spatial; ++l) TRY(layer_forward(pl.sp, l, l + 1 < p->n_spatial ? t.sp[l + 1].x : t.sp_out, dr, s));
  float* tp_dst = backbone_only ? logits : t.tp_out;  // where the temporal tower's output rows land
  float* g0 = p->n_temporal > 0 ? t.tp[0].x : tp_dst;
  const float* cls = t.sp_out;  // (frames, d) when the tail layer ran, else the CLS rows inside the token buffer: at stride N when padded
  const int64_t cls_stride = pl.sp.tail || ragged ? d : N * d;
  if (!pl.sp.tail && ragged) {  // CLS rows are not evenly strided: gather them (tp_out is free until the last temporal layer writes it)
    TRY(launch_gather_rows(t.sp_out, d, ix.f_cls_row, BT, d, t.tp_out, s));
    cls = t.tp_out;
  }
  TRY(launch_frames_embed(cls, cls_stride, in->frame_types, p->pos_emb, p->type_emb, p->frames_ln_w, p->frames_ln_b, p->ln_eps, B, T,
                          d, g0, s, t.s_frames, dr, ragged ? ix.f_orig : nullptr, BT));
  for (int64_t l = 0; l < p->n_temporal; ++l)
    TRY(layer_forward(pl.tp, l, l + 1 < p->n_temporal ? t.tp[l + 1].x : pl.tp.tail ? t.h0 : tp_dst, dr, s));
  if (backbone_only) return 0;
  if (!pl.tp.tail) TRY(launch_gather_rows(t.tp_out, d, ix.last_row, B, d, t.h0, s));                    // models.py:189-192
  TRY(launch_linear(t.h0, d, p->fc1_w, p->fc1_b, t.u0, d, B, d, d, STLT_ACT_NONE, s));
  TRY(launch_gelu_fwd(t.u0, t.z1, B * d, s));
  TRY(launch_add_layernorm(t.z1, d, nullptr, 0, p->head_ln_w, p->head_ln_b, p->ln_eps, B, d, t.z2, d, s));
  TRY(launch_linear(t.z2, d, p->fc2_w, p->fc2_b, logits, p->n_classes, B, p->n_classes, d, STLT_ACT_NONE, s));
  // the caller's row counts were taken on trust: NaN logits (hence a NaN loss) when they are not the index's or the masks break the contract
  return pl.host_counts ? launch_ragged_poison(ix, tok, BT, false, logits, B * p->n_classes, s) : 0;
}

int stlt_train_backward(const stlt_params* p, const stlt_params* g, const stlt_inputs* in, const void* tape_mem,
                        size_t tape_bytes, void* scratch_mem, size_t scratch_bytes, const float* dlogits,
                        float dropout_p, uint64_t dropout_seed, int flags, stlt_ctx* ctx, stlt_stream_t stream) {
  return stlt_train_backward_inputs(p, g, in, tape_mem, tape_bytes, scratch_mem, scratch_bytes, dlogits, dropout_p, dropout_seed, flags, ctx, nullptr,
                                    nullptr, stream);
}

// The same sweep, carried one step further: from the gradient wrt the pre-LayerNorm embedding sum to the gradient wrt the layout itself
// (what autograd gives the reference for batch["boxes"] / batch["scores"] as leaves, models.py:29-39).  Both outputs NULL: stlt_train_backward.
// (`maps`: stlt_train_backward_relevance's sinks — its caller has checked them — or nullptr, which is every other entry point)
static int reverse_sweep(const stlt_params* p, const stlt_params* g, const stlt_inputs* in, const void* tape_mem, size_t tape_bytes, void* scratch_mem,
                         size_t scratch_bytes, const float* dlogits, float dropout_p, uint64_t dropout_seed, int flags, stlt_ctx* ctx, float* d_boxes,
                         float* d_scores, const stlt_relevance_maps* maps, stlt_stream_t stream) {
  TRY(check_train(p, in, flags));
  if (!g || !dlogits || !tape_mem || !scratch_mem) return stlt_set_error(STLT_EINVAL, "stlt_train_backward: null argument");
  if (d_scores && !d_boxes) return stlt_set_error(STLT_EINVAL, "stlt_train_backward_inputs: d_scores comes with d_boxes");
  if (d_scores && !in->scores) return stlt_set_error(STLT_EINVAL, "stlt_train_backward_inputs: d_scores given but the inputs carry no scores");
  if (d_boxes && (flags & STLT_FLAG_TRAIN_UPPER_ONLY))
    return stlt_set_error(STLT_EINVAL, "stlt_train_backward_inputs: STLT_FLAG_TRAIN_UPPER_ONLY never reaches the embedding");
  if (const char* off = stlt_first_unaligned16({{"d_boxes", d_boxes}, {"d_scores", d_scores}}))
    return stlt_set_error(STLT_EINVAL, "stlt_train_backward_inputs: %s must be 16-byte aligned", off);
  const bool no_param_grads = grad_table_empty(p, g);
  hipStream_t s = (hipStream_t)stream;
  StltCtxScope ctx_scope(ctx, s);  // the sweep's input-gradient products may read the context's transposed weight copies
  if (ctx_scope.error()) return ctx_scope.error();
  const int64_t B = in->B, T = in->T, N = in->N, d = p->d, K = p->n_classes;
  Plan pl;
  TRY(plan_open(pl, p, in, tape_mem, tape_bytes, flags));
  const Tape& t = pl.t; const RaggedIndex& ix = pl.ix; const bool ragged = pl.ragged, backbone_only = pl.backbone_only;
  Scratch sc = scratch_layout((char*)scratch_mem, B, T, N, d, p->n_categories);
  if (scratch_bytes < sc.bytes) return stlt_set_error(STLT_EWORKSPACE, "scratch %zu B < required %zu B", scratch_bytes, sc.bytes);
  if ((uintptr_t)scratch_mem & 255) return stlt_set_error(STLT_EINVAL, "scratch must be 256-byte aligned");
  // the sweep's ~55 partial-row reductions (LayerNorm / bias gradients) are collected and run as a few batched launches
  // (STLT_TRAIN_DEFER_REDUCE=0: one launch each, A/B runs)
  StltReduceScope red(sc.red_pool, sc.red_pool_floats, sc.red, sc.red_floats, s);  // (no pool was carved while deferral is off)
  sc.rs = &red;
  StltGemmScratch gemm_scratch(sc.sk, STLT_GEMM_SCRATCH_BYTES);
  const StltDrop dr = stlt_drop_make(dropout_p, dropout_seed);
  const bool do_upper = !(flags & STLT_FLAG_TRAIN_LOWER_ONLY), do_lower = !(flags & STLT_FLAG_TRAIN_UPPER_ONLY);
  if (!do_upper && !do_lower) return stlt_set_error(STLT_EINVAL, "stlt_train_backward: UPPER_ONLY and LOWER_ONLY exclude each other");
  TRY(plan_rows(pl, p, in, false, s));
  const int64_t tok = pl.tok, BT = pl.BT;
  if (ragged) {
    if (N > AB_MAX_ROWS || T > AB_MAX_ROWS) return stlt_set_error(STLT_EINVAL, "attention backward supports sequences of at most %d tokens", AB_MAX_ROWS);
    TRY(launch_ragged_groups(ix, tok, BT, pl.fpg, s));
  }
  // (the fusion models' layout branch — STLT_FLAG_TRAIN_BACKBONE — keeps one stream: measured 43.75 against 44.1 ms per CACNF step at 64
  // clips; the block-level calls around the sweep are single-stream and the side launches only delay their small kernels)
  DwSide side = backbone_only || no_param_grads ? DwSide{} : dw_side_open(sc, ctx);
  DwSideHold side_hold(&side, s);
  DwQueue q_sp(&side, sc.sp), q_tp(&side, sc.tp);
  // Both schedules: the caller may hand in scratch that an earlier step with another (B,T,N) left dirty (two shapes can round to the same byte
  // count) and a ragged row count changes every step, so the operand rows beyond the row count are cleared every step.
  if (do_lower && !no_param_grads) TRY(clear_operand_padding(q_sp, pl.sp, s));
  if (do_upper && !no_param_grads) TRY(clear_operand_padding(q_tp, pl.tp, s));
  if (do_upper && backbone_only) {
    // the gradient of every row of the temporal tower's output arrives from the fusion layers: no head, no row gather
    if (hipError_t e = hipMemcpyAsync(sc.tp.A, dlogits, (size_t)BT * d * sizeof(float), hipMemcpyDeviceToDevice, s); e != hipSuccess)
      return stlt_set_error((int)e, "train_backward: copy: %s", hipGetErrorString(e));
    TRY(zero_rows(sc.tp.A, d, BT, pl.tp.Mp, s));
    const RelSink rel_tp{maps ? maps->abar_temporal : nullptr, p->n_spatial == 0};
    TRY(tower_backward(pl.tp, g->temporal, nullptr, sc.tp, sc, dr, s, q_tp, maps ? &rel_tp : nullptr));
  } else if (do_upper) {
  // ---- prediction head (models.py:162-163): logits = z2·W2ᵀ+b2, z2 = LN(z1), z1 = gelu(u0), u0 = h0·W1ᵀ+b1
  if (g->fc2_w) TRY(launch_small_gemm(dlogits, 1, K, t.z2, d, 1, stlt_grad(g->fc2_w), d, K, d, B, 1, s));   // (K,d) += dlogitsᵀ·z2
  if (g->fc2_b) TRY(launch_colsum_acc(dlogits, K, B, K, stlt_grad(g->fc2_b), red.chunk(), s));
  TRY(launch_small_gemm(dlogits, K, 1, p->fc2_w, d, 1, sc.hA, d, B, d, K, 0, s));                   // hA = dz2
  TRY(launch_ln_bwd(sc.hA, d, t.z1, d, nullptr, 0, p->head_ln_w, p->ln_eps, B, d, sc.hB, d, stlt_grad(g->head_ln_w), stlt_grad(g->head_ln_b),
                    red.chunk(), s));                                                                    // hB = dz1
  TRY(launch_gelu_bwd(sc.hB, t.u0, sc.hB, B * d, s));                                               // hB = du0
  // the two d x d products of fc1 go to the MFMA kernel (it contracts over multiples of 32 clips; the strided kernel takes the rest)
  if (g->fc1_w) {                                                                                   // (d,d) += du0ᵀ·h0
    const int64_t Bf = B / 32 * 32;
    if (Bf > 0) TRY(launch_gemm(1, 1, sc.hB, d, t.h0, d, nullptr, stlt_grad(g->fc1_w), d, stlt_grad(g->fc1_w), d, 0, d, d, Bf, 1, STLT_ACT_NONE, s));
    if (B > Bf) TRY(launch_small_gemm(sc.hB + Bf * d, 1, d, t.h0 + Bf * d, d, 1, stlt_grad(g->fc1_w), d, d, d, B - Bf, 1, s));
  }
  if (g->fc1_b) TRY(launch_colsum_acc(sc.hB, d, B, d, stlt_grad(g->fc1_b), red.chunk(), s));
  TRY(launch_gemm(0, 1, sc.hB, d, p->fc1_w, d, nullptr, nullptr, 0, sc.hA, d, 0, B, d, d, 1, STLT_ACT_NONE, s));  // hA = dh0
  // ---- temporal transformer: hA is the gradient wrt the last frame's row of every clip (models.py:189-192)
  const RelSink rel_tp{maps ? maps->abar_temporal : nullptr, p->n_spatial == 0};
  TRY(tower_backward(pl.tp, g->temporal, sc.hA, sc.tp, sc, dr, s, q_tp, maps ? &rel_tp : nullptr));
  }  // upper half: sc.tp.A now holds the gradient wrt the temporal tower's input
  if (!do_lower) { TRY(red.flush()); return dw_side_join(&side, s); }
  if (maps && p->n_spatial == 0) return relevance_finish(p, in, maps, red, s);  // no spatial map to sweep on for
  // ---- frames embeddings (models.py:98-111).  The gradient wrt the frames' CLS rows goes to tp.C, a chain-only buffer: the temporal
  // tower's last weight-gradient products may still be reading its operand sets on the side stream.
  float* d_cls = sc.tp.C;
  TRY(launch_ln_bwd(sc.tp.A, d, t.s_frames, d, nullptr, 0, p->frames_ln_w, p->ln_eps, BT, d, d_cls, d, stlt_grad(g->frames_ln_w),
                    stlt_grad(g->frames_ln_b), red.chunk(), s, dr, 0, nullptr, STLT_SITE_FRAMES));                // d_cls = gradient wrt the frames' CLS rows
  const bool dense_scatter = !ragged && !pl.sp.tail;  // padded dense schedule: the CLS rows sit at stride N in the token buffer
  TRY(launch_frames_bwd(d_cls, in->frame_types, B, T, N, d, dense_scatter ? sc.sp.A : nullptr, stlt_grad(g->pos_emb), stlt_grad(g->type_emb), red.chunk(), s,
                        ragged ? ix.f_row_of : nullptr, !no_param_grads));
  // ---- spatial transformer (its queue flushes per layer)
  const RelSink rel_sp{maps ? maps->abar_spatial : nullptr, true};
  TRY(tower_backward(pl.sp, g->spatial, dense_scatter ? nullptr : d_cls, sc.sp, sc, dr, s, q_sp, maps ? &rel_sp : nullptr));
  if (maps) return relevance_finish(p, in, maps, red, s);  // the layer-0 input product and the embedding backward are not needed
  // ---- category / box / score embeddings (models.py:29-39); sp.C for the same reason as tp.C above
  TRY(launch_ln_bwd(sc.sp.A, d, t.s_embed, d, nullptr, 0, p->emb_ln_w, p->ln_eps, tok, d, sc.sp.C, d, stlt_grad(g->emb_ln_w), stlt_grad(g->emb_ln_b),
                    red.chunk(), s, dr, 0, nullptr, STLT_SITE_EMBED));
  if (!no_param_grads)
    TRY(launch_embed_bwd(sc.sp.C, in->categories, in->boxes, in->scores, p->n_categories, tok, d, stlt_grad(g->cat_emb), stlt_grad(g->box_w),
                         stlt_grad(g->box_b), stlt_grad(g->score_w), stlt_grad(g->score_b), red.chunk(), s, ragged ? ix.t_orig : nullptr));
  if (d_boxes)
    TRY(launch_embed_bwd_inputs(sc.sp.C, p->box_w, d_scores ? p->score_w : nullptr, tok, d, d_boxes, d_scores, B * T * N, s, ragged ? ix.t_orig : nullptr));
  TRY(red.flush());
  return dw_side_join(&side, s);
}

int stlt_train_backward_inputs(const stlt_params* p, const stlt_params* g, const stlt_inputs* in, const void* tape_mem,
                               size_t tape_bytes, void* scratch_mem, size_t scratch_bytes, const float* dlogits,
                               float dropout_p, uint64_t dropout_seed, int flags, stlt_ctx* ctx, float* d_boxes, float* d_scores,
                               stlt_stream_t stream) {
  return reverse_sweep(p, g, in, tape_mem, tape_bytes, scratch_mem, scratch_bytes, dlogits, dropout_p, dropout_seed, flags, ctx, d_boxes, d_scores, nullptr,
                       stream);
}

// Attention relevance of a prediction: the input-only sweep (an all-NULL gradient table: no weight-gradient product, no parameter reduction,
// no side stream) with one stlt_attn_grad_probs launch in front of every attention backward, then the two rollouts and the combine (the fusion
// models' layout branch, STLT_FLAG_TRAIN_BACKBONE: from the gradient of the backbone's output, and without the combine).
int stlt_train_backward_relevance(const stlt_params* p, const stlt_inputs* in, const void* tape_mem, size_t tape_bytes, void* scratch_mem,
                                  size_t scratch_bytes, const float* dlogits, float dropout_p, uint64_t dropout_seed, int flags, stlt_ctx* ctx,
                                  const stlt_relevance_maps* maps, stlt_stream_t stream) {
  TRY(check_train(p, in, flags));
  if (!maps) return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: null maps");
  if (flags & STLT_FLAG_SKIP_PADDING)
    return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: STLT_FLAG_SKIP_PADDING is not supported (the maps have the padded geometry)");
  if (flags & (STLT_FLAG_TRAIN_UPPER_ONLY | STLT_FLAG_TRAIN_LOWER_ONLY))
    return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: the relevance needs the whole sweep of both towers (no UPPER_ONLY / LOWER_ONLY)");
  const bool backbone = (flags & STLT_FLAG_TRAIN_BACKBONE) != 0;  // the seed is the (B,T,d) gradient of the backbone's output, as in stlt_train_backward
  if (backbone && maps->relevance)
    return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: relevance must be NULL with STLT_FLAG_TRAIN_BACKBONE (stlt_relevance_combine_joint reads the rollouts out)");
  if (dropout_p != 0.f) return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: dropout_p must be 0 (the gradient wrt the probabilities is defined with dropout off)");
  if (in->N > AB_MAX_ROWS || in->T > AB_MAX_ROWS)
    return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: sequences of at most %d tokens (N=%lld, T=%lld)", AB_MAX_ROWS, (long long)in->N, (long long)in->T);
  if (!maps->rollout_spatial || !maps->rollout_temporal || (!backbone && !maps->relevance) || (p->n_spatial > 0 && !maps->abar_spatial) || (p->n_temporal > 0 && !maps->abar_temporal))
    return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: null map (abar_spatial / abar_temporal may be NULL only for a tower without layers)");
  for (const StltNamedPtr& q : {StltNamedPtr{"abar_spatial", maps->abar_spatial}, StltNamedPtr{"abar_temporal", maps->abar_temporal},
                                StltNamedPtr{"rollout_spatial", maps->rollout_spatial}, StltNamedPtr{"rollout_temporal", maps->rollout_temporal},
                                StltNamedPtr{"relevance", maps->relevance}})
    if ((uintptr_t)q.p & 3) return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: %s must be 4-byte aligned", q.name);
  if ((uintptr_t)in->lengths & 7) return stlt_set_error(STLT_EINVAL, "stlt_train_backward_relevance: lengths must be 8-byte aligned");
  const stlt_params none{};  // names no parameter gradient at all
  return reverse_sweep(p, &none, in, tape_mem, tape_bytes, scratch_mem, scratch_bytes, dlogits, 0.f, dropout_seed, flags, ctx, nullptr, nullptr, maps, stream);
}

}  // extern "C"
