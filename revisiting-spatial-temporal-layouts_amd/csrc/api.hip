// C-ABI of libstlt_hip.so (see include/stlt_hip.h): argument checks, error string, per-kernel event
// timing, and the whole-path orchestration (StltBackbone.forward / Stlt.forward as a fixed launch sequence
// on the caller's stream — no allocation, no synchronisation, graph-capturable).
// The inference schedule is written once: ws_carve (the workspace checks and the typed buffers of every entry point), spatial_tower and
// temporal_tower (the layer loops), LayerOpts (what a forward adds per layer: stlt_forward_attention is the dense schedule with `unfused`
// and a probabilities sink), classification_head.  Two schedules stand beside it on the same carve: forward_ragged (skip-padding) and
// the two-stream temporal loop of stlt_forward_prefixes.
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"

namespace {
thread_local char g_err[512] = "";

// Per-kernel timing: the switch is process-wide, the records and the event pool are per device (an event belongs to the
// device it was created on), and a launch's two events are recorded on the launch's own stream.
struct ProfRec { int kid; hipEvent_t a, b; double flops, bytes; int kernels; char note[STLT_PROF_NOTE]; };
thread_local char t_note[STLT_PROF_NOTE] = "";
thread_local double t_flops = 0.0, t_bytes = 0.0;
thread_local int t_kernels = 0;  // kernel launches checked (stlt_check_launch) inside the open scope
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs[STLT_MAX_DEVICES];
std::vector<hipEvent_t> g_event_pool[STLT_MAX_DEVICES];
thread_local hipEvent_t g_open_start = nullptr;
thread_local int g_scope_depth = 0;
double g_gemm_flops[STLT_MAX_DEVICES] = {};

hipEvent_t get_event(int dev) {
  auto& pool = g_event_pool[dev];
  if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
StltPerDeviceInt g_cus;
}  // namespace

int stlt_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  return dev;
}

int stlt_device_cus() {
  int& n = g_cus.ref();
  if (n == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, stlt_current_device()) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}

int stlt_set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int stlt_check_launch(const char* what) {
  if (g_scope_depth > 0) ++t_kernels;
  else if (g_prof_on) {  // a kernel outside every scope still gets a record (no events: 0 us), so that the records cover every kernel the library starts
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfRec rec{STLT_K_MISC, nullptr, nullptr, 0.0, 0.0, 1, {0}};
    snprintf(rec.note, sizeof(rec.note), "%s (outside the recorder's scopes)", what);
    g_prof_recs[stlt_current_device() & (STLT_MAX_DEVICES - 1)].push_back(rec);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return stlt_set_error((int)e, "%s: %s", what, hipGetErrorString(e));
  return 0;
}

void stlt_prof_begin(int kid, hipStream_t s) {
  if (g_scope_depth++ > 0) return;  // nested launcher: the outer scope times it
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_open_start = get_event(stlt_current_device() & (STLT_MAX_DEVICES - 1));
  t_note[0] = 0;
  t_flops = t_bytes = 0.0;
  t_kernels = 0;
  (void)hipEventRecord(g_open_start, s);
}

void stlt_prof_add_flops(double flops) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_gemm_flops[stlt_current_device() & (STLT_MAX_DEVICES - 1)] += flops;
  t_flops += flops;
}

// What the open (outermost) scope's launch is: shape, tile, workgroups, rounds, k-steps — appended to the launch's record for
// stlt_prof_launches (tools/launch_bound.py prices every launch of a step against its own bound).  Free when the recorder is off.
void stlt_prof_note(const char* fmt, ...) {
  if (!g_prof_on || g_scope_depth == 0 || !g_open_start) return;
  const size_t used = strlen(t_note);
  if (used + 2 >= sizeof(t_note)) return;
  if (used) { t_note[used] = ' '; t_note[used + 1] = 0; }
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(t_note + strlen(t_note), sizeof(t_note) - strlen(t_note), fmt, ap);
  va_end(ap);
}
void stlt_prof_add_bytes(double bytes) {
  if (g_prof_on && g_scope_depth > 0) t_bytes += bytes;
}
// FLOPs of a launch that is not a matrix-core product of the GEMM roofline (fused MHSA, attention cores): on the launch's record only
void stlt_prof_note_flops(double flops) {
  if (g_prof_on && g_scope_depth > 0) t_flops += flops;
}

void stlt_prof_end(int kid, hipStream_t s) {
  if (--g_scope_depth > 0) return;
  if (!g_prof_on || !g_open_start) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  const int dev = stlt_current_device() & (STLT_MAX_DEVICES - 1);
  hipEvent_t b = get_event(dev);
  (void)hipEventRecord(b, s);
  ProfRec rec{kid, g_open_start, b, t_flops, t_bytes, t_kernels, {0}};
  memcpy(rec.note, t_note, sizeof(rec.note));
  g_prof_recs[dev].push_back(rec);
  g_open_start = nullptr;
}

unsigned long long* g_stlt_debug_buf = nullptr;

// Layers whose sequences have at most 64 tokens (and 64-channel heads) run the in-projection and the attention core as ONE kernel
// (mhsa.hip: the packed QKV tensor never reaches HBM).  Round 3 had this for 32-frame clips only; round 4's kernel takes the
// reference's real layouts (T = 17 / 33, datasets.py:97-113), cfg4's 64 frames and the training forward.  STLT_FUSED_MHSA=0
// restores the two launches everywhere, STLT_FUSED_MHSA_SPATIAL=0 for the spatial tower's (non-causal) layers only (A/B runs).
bool stlt_fused_mhsa_on(int causal) {
  static const bool on = [] { const char* e = getenv("STLT_FUSED_MHSA"); return e ? atoi(e) != 0 : true; }();
  static const bool spatial = [] { const char* e = getenv("STLT_FUSED_MHSA_SPATIAL"); return e ? atoi(e) != 0 : true; }();
  return on && (causal || spatial);
}

extern "C" {

int stlt_debug_set_buffer(void* dev_buf) { g_stlt_debug_buf = (unsigned long long*)dev_buf; return 0; }
size_t stlt_debug_buffer_bytes(void) { return ((size_t)54 * (size_t)stlt_device_cus() + 1024) * sizeof(unsigned long long); }

int stlt_version(void) { return STLT_VERSION; }
const char* stlt_last_error(void) { return g_err; }

int stlt_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
  return 0;
}

double stlt_prof_take_gemm_flops(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double& f = g_gemm_flops[stlt_current_device() & (STLT_MAX_DEVICES - 1)];
  const double out = f;
  f = 0.0;
  return out;
}

int stlt_prof_collect(double* ms_out, int64_t* launches_out) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int k = 0; k < STLT_K_COUNT; ++k) { if (ms_out) ms_out[k] = 0.0; if (launches_out) launches_out[k] = 0; }
  const int dev = stlt_current_device() & (STLT_MAX_DEVICES - 1);  // the records of the device that is current
  for (auto& r : g_prof_recs[dev]) {
    if (!r.a) continue;  // a kernel outside the scopes: counted by stlt_prof_launches only
    hipError_t e = hipEventSynchronize(r.b);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, r.a, r.b);
    if (e != hipSuccess) return stlt_set_error((int)e, "stlt_prof_collect: %s", hipGetErrorString(e));
    if (r.kid >= 0 && r.kid < STLT_K_COUNT) { if (ms_out) ms_out[r.kid] += ms; if (launches_out) launches_out[r.kid] += 1; }
    g_event_pool[dev].push_back(r.a);
    g_event_pool[dev].push_back(r.b);
  }
  g_prof_recs[dev].clear();
  return 0;
}

int stlt_prof_launches(stlt_prof_launch* out, int64_t cap, int64_t* n_out) {
  if (!n_out || (cap > 0 && !out)) return stlt_set_error(STLT_EINVAL, "stlt_prof_launches: null argument");
  std::lock_guard<std::mutex> lk(g_prof_mu);
  const int dev = stlt_current_device() & (STLT_MAX_DEVICES - 1);
  int64_t n = 0;
  for (auto& r : g_prof_recs[dev]) {
    hipError_t e = hipSuccess;
    float ms = 0.f;
    if (r.a) {
      e = hipEventSynchronize(r.b);
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, r.a, r.b);
    }
    if (e != hipSuccess) return stlt_set_error((int)e, "stlt_prof_launches: %s", hipGetErrorString(e));
    if (n < cap) {
      out[n].kid = r.kid; out[n].kernels = r.kernels; out[n].us = ms * 1e3f; out[n].flops = r.flops; out[n].bytes = r.bytes;
      memcpy(out[n].note, r.note, sizeof(out[n].note));
      out[n].note[sizeof(out[n].note) - 1] = 0;
    }
    ++n;
    if (r.a) { g_event_pool[dev].push_back(r.a); g_event_pool[dev].push_back(r.b); }
  }
  g_prof_recs[dev].clear();
  *n_out = n;
  return 0;
}

int stlt_embed_fwd(const int64_t* categories, const float* boxes, const float* scores, const float* cat_table,
                   int64_t n_categories, const float* box_w, const float* box_b, const float* score_w,
                   const float* score_b, const float* ln_w, const float* ln_b, float eps, int64_t n_tokens, int64_t d,
                   float* out, stlt_stream_t stream) {
  return launch_embed(categories, boxes, scores, cat_table, n_categories, box_w, box_b, score_w, score_b, ln_w, ln_b,
                      eps, n_tokens, d, out, (hipStream_t)stream);
}

int stlt_linear_fwd(const float* x, int64_t ldx, const float* w, const float* bias, float* y, int64_t ldy, int64_t M,
                    int64_t N, int64_t K, int act, stlt_stream_t stream) {
  return launch_linear(x, ldx, w, bias, y, ldy, M, N, K, act, (hipStream_t)stream);
}

int stlt_linear_small_fwd(const float* x, int64_t ldx, const float* w, const float* bias, const float* r, int64_t ldr, float* y, int64_t ldy, int64_t M,
                          int64_t N, int64_t K, int act, int tile, stlt_stream_t stream) {
  const int code = stlt_gemm16_tile_from_public(tile);
  if (code == 0) return stlt_set_error(STLT_EINVAL, "stlt_linear_small_fwd: tile = columns | rows << 16: 128 rows (or 0) x {48,64,96,128,144,192}, 64 x {64,96,128,160,192,256}, 32 x {128,192,256}");
  bool taken = false;
  if (int e = launch_linear_gemm16(x, ldx, w, K, bias, r, ldr, y, ldy, M, N, K, act, (hipStream_t)stream, &taken, code)) return e;
  return taken || M == 0 ? 0 : stlt_set_error(STLT_EINVAL, "stlt_linear_small_fwd: shape or activation not taken by the small-tile kernel");
}

int stlt_input_grad_small(const float* dy, int64_t ld_dy, const float* w, int64_t n_out, int64_t k_in, const float* r, int64_t ldr, float* dx, int64_t ld_dx,
                          int64_t M, int tile, stlt_ctx* ctx, stlt_stream_t stream) {
  // tile 0: routed by the launch-time estimate, and — when `ctx` holds a current transposed copy of w — run as a forward product on the copy
  const int code = tile == 0 ? 0 : stlt_gemm16_tile_from_public(tile);
  if (tile != 0 && code == 0) return stlt_set_error(STLT_EINVAL, "stlt_input_grad_small: tile = 0 (by estimate) or columns | rows << 16: 128 rows (or 0) x {48,64,96,128,144,192}, 64 x {64,96,128,160,192,256}, 32 x {128,192,256}");
  StltCtxScope ctx_scope(ctx, (hipStream_t)stream);
  if (ctx_scope.error()) return ctx_scope.error();
  bool taken = false;
  if (int e = launch_input_grad_gemm16(dy, ld_dy, w, n_out, k_in, r, ldr, dx, ld_dx, M, (hipStream_t)stream, &taken, code)) return e;
  return taken || M == 0 ? 0 : stlt_set_error(STLT_EINVAL, "stlt_input_grad_small: shape not taken by the small-tile kernel");
}

int stlt_linear_small_choice(int64_t M, int64_t N, int64_t K) { return stlt_gemm16_tile_to_public(stlt_gemm16_choice(M, N, K, K, K)); }
int stlt_input_grad_small_choice(int64_t M, int64_t n_out, int64_t k_in) { return stlt_gemm16_tile_to_public(stlt_gemm16_choice(M, k_in, n_out, n_out, k_in, true)); }
int stlt_set_gemm_small_tiles(int mode) { return stlt_gemm16_set_mode(mode); }

int stlt_gemm(int transA, int transB, const float* a, int64_t lda, const float* b, int64_t ldb, const float* r, int64_t ldr,
              float* c, int64_t ldc, int64_t slab_stride, int64_t M, int64_t N, int64_t K, int n_split,
              stlt_stream_t stream) {
  return launch_gemm(transA, transB, a, lda, b, ldb, nullptr, r, ldr, c, ldc, slab_stride, M, N, K, n_split,
                     STLT_ACT_NONE, (hipStream_t)stream);
}

int stlt_weight_grad_group(const stlt_wgrad_item* items, int n_items, stlt_stream_t stream) {
  static_assert(sizeof(stlt_wgrad_item) == sizeof(StltWeightGradItem), "the C-ABI item is the internal item");
  return launch_weight_grad_group(reinterpret_cast<const StltWeightGradItem*>(items), n_items, (hipStream_t)stream);
}

size_t stlt_gemm_scratch_bytes(void) { return STLT_GEMM_SCRATCH_BYTES; }

int stlt_gemm_set_scratch(void* scratch, size_t bytes) {
  if (scratch && bytes < STLT_GEMM_SCRATCH_BYTES)
    return stlt_set_error(STLT_EWORKSPACE, "gemm scratch %zu B < required %zu B", bytes, (size_t)STLT_GEMM_SCRATCH_BYTES);
  if ((uintptr_t)scratch & 15) return stlt_set_error(STLT_EINVAL, "stlt_gemm_set_scratch: scratch must be 16-byte aligned (partial tiles are 16-byte stores)");
  stlt_gemm_set_scratch_impl(scratch, bytes);
  return 0;
}

int stlt_reduce_slabs(const float* slabs, int64_t stride, int n_slabs, float* dst, int64_t n, int accumulate,
                      stlt_stream_t stream) {
  StltProfScope ps(STLT_K_MISC, (hipStream_t)stream);  // a record of its own: the launcher's note (its cut) is kept
  return launch_reduce_slabs(slabs, stride, n_slabs, dst, n, accumulate, (hipStream_t)stream);
}

int stlt_attn_core_fwd(const float* qkv, const uint8_t* kpm, int causal, int64_t S, int64_t L, int64_t H, int64_t dh,
                       float* ctx, stlt_stream_t stream) {
  return launch_attn(qkv, kpm, causal, S, L, H, dh, ctx, causal ? STLT_K_ATTN_TEMPORAL : STLT_K_ATTN_SPATIAL,
                     (hipStream_t)stream);
}

int stlt_fused_mhsa_active(int64_t T, int64_t d, int64_t H) { return (stlt_fused_mhsa_on(1) && stlt_mhsa_fused_pays(1024, T, H, d, 1)) ? 1 : 0; }
int stlt_fused_mhsa_used(int64_t S, int64_t L, int64_t d, int64_t H, int causal) { return (stlt_fused_mhsa_on(causal) && stlt_mhsa_fused_pays(S, L, H, d, causal)) ? 1 : 0; }

int stlt_mhsa_fused_fwd(const float* x, const float* in_proj_w, const float* in_proj_b, const uint8_t* kpm, int64_t S, int64_t L, int64_t H,
                        int64_t d, float* ctx, stlt_stream_t stream) {
  return launch_mhsa_fused(x, in_proj_w, in_proj_b, kpm, S, L, H, d, ctx, (hipStream_t)stream);
}

int stlt_mhsa_fused_fwd_ex(const float* x, const float* in_proj_w, const float* in_proj_b, const uint8_t* kpm, int causal, int64_t S, int64_t L,
                           int64_t H, int64_t d, float dropout_p, uint64_t seed, uint32_t site, float* ctx, float* qkv_out, stlt_stream_t stream) {
  if (dropout_p < 0.f || dropout_p >= 1.f) return stlt_set_error(STLT_EINVAL, "stlt_mhsa_fused_fwd_ex: dropout_p must be in [0, 1)");
  return launch_mhsa_fused(x, in_proj_w, in_proj_b, kpm, S, L, H, d, ctx, (hipStream_t)stream, causal, qkv_out, stlt_drop_make(dropout_p, seed), site);
}

int stlt_attn_cross_fwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const uint8_t* kpm, int causal,
                        int64_t S, int64_t Lq, int64_t Lk, int64_t H, int64_t dh, float* ctx, stlt_stream_t stream) {
  return launch_attn_general(q, ldq, k, v, ldkv, kpm, causal, S, Lq, Lk, H, dh, ctx,
                             causal ? STLT_K_ATTN_TEMPORAL : STLT_K_ATTN_SPATIAL, (hipStream_t)stream);
}

int stlt_attn_ragged_fwd(const float* qkv, const int32_t* seg_start, const int32_t* seg_end, int causal, int64_t M, int64_t H,
                         int64_t dh, float* ctx, stlt_stream_t stream) {
  return launch_attn_ragged(qkv, seg_start, seg_end, causal, M, H, dh, ctx, causal ? STLT_K_ATTN_TEMPORAL : STLT_K_ATTN_SPATIAL,
                            (hipStream_t)stream);
}

int stlt_add_layernorm_fwd(const float* x, int64_t ldx, const float* res, int64_t ldres, const float* ln_w,
                           const float* ln_b, float eps, int64_t M, int64_t d, float* out, int64_t ldout,
                           stlt_stream_t stream) {
  return launch_add_layernorm(x, ldx, res, ldres, ln_w, ln_b, eps, M, d, out, ldout, (hipStream_t)stream);
}

int stlt_frames_embed_fwd(const float* spatial, int64_t row_stride, const int64_t* frame_types, const float* pos_table,
                          const float* type_table, const float* ln_w, const float* ln_b, float eps, int64_t B,
                          int64_t T, int64_t d, float* out, stlt_stream_t stream) {
  return launch_frames_embed(spatial, row_stride, frame_types, pos_table, type_table, ln_w, ln_b, eps, B, T, d, out,
                             (hipStream_t)stream);
}

int stlt_gather_last_fwd(const float* x, const int64_t* lengths, int64_t B, int64_t T, int64_t d, float* out,
                         stlt_stream_t stream) {
  return launch_gather_last(x, lengths, B, T, d, out, (hipStream_t)stream);
}

// ------------------------------------------------------------------ whole path

}  // extern "C"

struct WsLayout {
  size_t x, x1, qkv, ctx, tmp, hh, head, sk, ridx, total;
};

// min_slots: rows per frame the buffers hold at least (the per-prefix forward runs two temporal streams: 2 rows per frame)
static WsLayout ws_layout(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_classes, int64_t min_slots) {
  const size_t tok = (size_t)B * T * (N > min_slots ? N : min_slots);  // spatial tokens >= temporal tokens
  const size_t f = sizeof(float);
  WsLayout w;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = stlt_align256(off + bytes); return o; };
  w.x = take(tok * d * f);
  w.x1 = take(tok * d * f);
  w.qkv = take(tok * 3 * d * f);
  w.ctx = take(tok * d * f);
  w.tmp = take(tok * d * f);
  w.hh = take(tok * 4 * d * f);
  w.head = take((size_t)B * (3 * d + (n_classes < 0 ? 0 : n_classes)) * f);
  w.sk = take(STLT_GEMM_SCRATCH_BYTES);  // stream-K partial tiles of under-filled GEMM launches
  w.ridx = take(ragged_index_bytes(B, T, N));  // STLT_FLAG_SKIP_PADDING: index of the real tokens / frames
  w.total = off;
  return w;
}

// The one workspace size (declared in common.h: caf.hip places a backbone workspace inside its own); the exported size functions add
// their treatment of empty shapes
size_t stlt_ws_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_classes, int64_t min_slots) {
  return ws_layout(B, T, N, d, n_classes, min_slots).total;
}

// The carved workspace: x, x1, ctx, tmp hold (tok, d) floats, qkv 3x and hh 4x as wide; head the classification head's rows; sk the
// stream-K scratch an entry point lends to its GEMMs (StltGemmScratch); ridx the skip-padding index.
struct WsBufs {
  float *x, *x1, *qkv, *ctx, *tmp, *hh, *head;
  char *sk, *ridx;
};

// The workspace checks of every whole-path entry point, then the carve.  short_code / who: what a short workspace returns and how its
// message opens (stlt_forward_attention documents STLT_EINVAL under its own name; every other entry point STLT_EWORKSPACE, no name).
static int ws_carve(const stlt_params* p, const stlt_inputs* in, int64_t min_slots, void* workspace, size_t workspace_bytes, int short_code,
                    const char* who, WsBufs* b) {
  const WsLayout w = ws_layout(in->B, in->T, in->N, p->d, p->n_classes, min_slots);
  if (!workspace || workspace_bytes < w.total) return stlt_set_error(short_code, "%sworkspace %zu B < required %zu B", who, workspace_bytes, w.total);
  if ((uintptr_t)workspace & 255) return stlt_set_error(STLT_EINVAL, "workspace must be 256-byte aligned");
  char* base = (char*)workspace;
  auto F = [&](size_t o) { return (float*)(base + o); };
  *b = WsBufs{F(w.x), F(w.x1), F(w.qkv), F(w.ctx), F(w.tmp), F(w.hh), F(w.head), base + w.sk, base + w.ridx};
  return 0;
}

// The residual adds of a post-norm layer ride in the out-proj / FFN2 epilogues and the LayerNorm passes read one tensor
// instead of two (bit-identical logits: the bias joins the finished sum, the residual is added last).  Round 2 measured
// it a wash (the residual tile was read inside the exposed epilogue: LayerNorm 3.06 -> 2.00 ms, GEMMs +1.0 ms); with the
// first half of a tile's residual pieces requested during the tile's last k-step (gemm.hip: RES_PF) the GEMMs
// pay 0.4 ms and the forward gains 0.5 ms at cfg2 / 1024 clips (profiles/round3_fwd_residual_ab.txt).  STLT_FUSE_RESIDUAL=0
// restores the separate pass (A/B runs).
static bool fuse_residual() {
  static const bool on = [] { const char* e = getenv("STLT_FUSE_RESIDUAL"); return e ? atoi(e) != 0 : true; }();
  return on;
}

// What a padded layer does beyond the plain forward.  unfused: never the fused launch, the packed QKV lies in the workspace.  probs != null
// (needs unfused): the layer's attention probabilities, (S,L,L) or per_head (S,H,L,L), written by launch_attn_probs right behind the core.
struct LayerOpts {
  bool unfused = false;
  float* probs = nullptr;
  int per_head = 0;
};

// in-projection + attention core of a layer: ctx (M,d) from x (M,d).  seg_start / seg_end != null: the M rows are compacted rows cut
// into variable-length segments (ragged.hip) and the attention is restricted to the row's own segment (no padded keys exist; S, L and
// kpm are not read); that form never takes the fused launch and takes no options.
static int qkv_attention(const stlt_layer_params& lp, int64_t d, int64_t H, const float* x, int64_t M, int64_t S, int64_t L,
                         const uint8_t* kpm, const int* seg_start, const int* seg_end, int causal, int kid, float* qkv, float* ctx,
                         hipStream_t s, const LayerOpts& o = {}) {
  // with the opt-in split-bf16 products on, a temporal in-projection they take is faster as its own launch (+ the attention core)
  // than inside the fused f32-MFMA kernel
  if (!seg_start && !o.unfused && stlt_fused_mhsa_on(causal) && stlt_mhsa_fused_pays(S, L, H, d, causal) && !stlt_split_bf16_takes(M, 3 * d, d, d, d))
    return launch_mhsa_fused(x, lp.in_proj_w, lp.in_proj_b, kpm, S, L, H, d, ctx, s, causal);
  TRY(launch_linear(x, d, lp.in_proj_w, lp.in_proj_b, qkv, 3 * d, M, 3 * d, d, STLT_ACT_NONE, s));
  if (seg_start) return launch_attn_ragged(qkv, seg_start, seg_end, causal, M, H, d / H, ctx, kid, s);
  TRY(launch_attn(qkv, kpm, causal, S, L, H, d / H, ctx, kid, s));
  return o.probs ? launch_attn_probs(qkv, kpm, causal, S, L, H, d / H, o.per_head, o.probs, s) : 0;
}

// Layer l's options out of a tower's: its own (S,L,L) or (S,H,L,L) maps of the sink
static LayerOpts layer_opts(LayerOpts o, int64_t l, int64_t S, int64_t L, int64_t H) {
  if (o.probs) o.probs += (size_t)l * S * (o.per_head ? H : 1) * L * L;
  return o;
}

// The part of a post-norm encoder layer (nn.TransformerEncoderLayer as configured at models.py:46-52,118-124) behind the attention
// core, on M rows of width d: ctx (stride ldctx) holds their attention outputs, x (stride ldx) their layer inputs.  x1 (M,d) receives
// the post-norm1 rows.  `out` may alias `x` (x is last read by the norm1 residual) or `ctx` (last read by the out-projection); x1 must not.
static int encoder_tail(const stlt_layer_params& lp, int64_t d, const float* ctx, int64_t ldctx, const float* x, int64_t ldx, int64_t M,
                        bool fuse, float* tmp, float* x1, float* hh, float* out, hipStream_t s) {
  TRY(stlt_linear_add_norm(ctx, ldctx, d, lp.out_proj_w, lp.out_proj_b, x, ldx, lp.norm1_w, lp.norm1_b, 1e-5f, M, d, fuse, tmp, x1, s));
  return stlt_ffn_norm(x1, d, lp.lin1_w, lp.lin1_b, STLT_ACT_GELU, lp.lin2_w, lp.lin2_b, lp.norm2_w, lp.norm2_b, 1e-5f, M, d, fuse, hh, tmp, out, s);
}

// One post-norm encoder layer on M compact rows of width d, padded layout or (seg_start / seg_end) ragged.  Aliasing as encoder_tail.
static int encoder_layer(const stlt_layer_params& lp, int64_t d, int64_t H, const float* x, int64_t M, int64_t S, int64_t L,
                         const uint8_t* kpm, const int* seg_start, const int* seg_end, int causal, int kid, float* qkv, float* ctx,
                         float* tmp, float* x1, float* hh, float* out, hipStream_t s, const LayerOpts& o = {}) {
  TRY(qkv_attention(lp, d, H, x, M, S, L, kpm, seg_start, seg_end, causal, kid, qkv, ctx, s, o));
  return encoder_tail(lp, d, ctx, d, x, d, M, fuse_residual(), tmp, x1, hh, out, s);
}

static int check_params(const stlt_params* p, const stlt_inputs* in, bool need_head) {
  if (!p || !in) return stlt_set_error(STLT_EINVAL, "null params/inputs");
  if (!stlt_heads_ok(p->d, p->H))
    return stlt_set_error(STLT_EINVAL, "hidden_size %lld / heads %lld: need hidden_size %% heads == 0, a head dim of at most 256 and hidden_size %% 4 == 0", (long long)p->d, (long long)p->H);
  if (in->B <= 0 || in->T <= 0 || in->N <= 0) return stlt_set_error(STLT_EINVAL, "empty batch (B=%lld,T=%lld,N=%lld)", (long long)in->B, (long long)in->T, (long long)in->N);
  if (in->T > p->n_positions) return stlt_set_error(STLT_EINVAL, "T=%lld exceeds the position table (%lld rows)", (long long)in->T, (long long)p->n_positions);
  if (!in->categories || !in->boxes || !in->kpm_boxes || !in->frame_types || !in->kpm_frames)
    return stlt_set_error(STLT_EINVAL, "null input tensor");
  if (p->n_spatial < 0 || p->n_temporal < 0 || (p->n_spatial && !p->spatial) || (p->n_temporal && !p->temporal))
    return stlt_set_error(STLT_EINVAL, "layer tables missing");
  if (need_head && (!p->fc1_w || !p->fc1_b || !p->head_ln_w || !p->head_ln_b || !p->fc2_w || !p->fc2_b || !in->lengths || p->n_classes <= 0))
    return stlt_set_error(STLT_EINVAL, "prediction head parameters / lengths missing");
  return 0;
}

// ------------------------------------------------------------------ the post-norm block, written once (declared in common.h)
// Every forward of the library ends its half-blocks and its heads here; the callers keep their projections, attention launches, gathers
// and buffers (and their aliasing contracts).  No profiling scope, no GEMM scratch, no memory of their own.

int stlt_linear_add_norm(const float* x, int64_t ldx, int64_t K, const float* w, const float* b, const float* res, int64_t ldres,
                         const float* ln_w, const float* ln_b, float eps, int64_t M, int64_t d, bool fuse, float* tmp, float* out,
                         hipStream_t s) {
  if (fuse) {  // the residual add rides in the product's epilogue: the norm pass reads one tensor
    TRY(launch_linear_add(x, ldx, w, b, res, ldres, tmp, d, M, d, K, s));
    return launch_add_layernorm(tmp, d, nullptr, 0, ln_w, ln_b, eps, M, d, out, d, s);
  }
  TRY(launch_linear(x, ldx, w, b, tmp, d, M, d, K, STLT_ACT_NONE, s));
  return launch_add_layernorm(tmp, d, res, ldres, ln_w, ln_b, eps, M, d, out, d, s);
}

int stlt_ffn_norm(const float* x, int64_t ldx, const float* w1, const float* b1, int act, const float* w2, const float* b2,
                  const float* ln_w, const float* ln_b, float eps, int64_t M, int64_t d, bool fuse, float* hh, float* tmp, float* out,
                  hipStream_t s) {
  TRY(launch_linear(x, ldx, w1, b1, hh, 4 * d, M, 4 * d, d, act, s));
  return stlt_linear_add_norm(hh, 4 * d, 4 * d, w2, b2, x, ldx, ln_w, ln_b, eps, M, d, fuse, tmp, out, s);
}

int stlt_head(const stlt_head_params& h, const float* x, int64_t ldx, int64_t in_dim, int64_t B, int64_t d, int64_t K, float eps,
              float* h1, float* h2, float* logits, hipStream_t s) {
  TRY(launch_linear(x, ldx, h.fc1_w, h.fc1_b, h1, d, B, d, in_dim, STLT_ACT_GELU, s));  // gelu(fc1(x))
  TRY(launch_add_layernorm(h1, d, nullptr, 0, h.ln_w, h.ln_b, eps, B, d, h2, d, s));
  return launch_linear(h2, d, h.fc2_w, h.fc2_b, logits, K, B, K, d, STLT_ACT_NONE, s);
}

// The model's own ClassificationHead on n rows of x (n,d); h1, h2: (n,d)
static int classification_head(const stlt_params* p, const float* x, int64_t n, float* h1, float* h2, float* logits, hipStream_t s) {
  const stlt_head_params head{p->fc1_w, p->fc1_b, p->head_ln_w, p->head_ln_b, p->fc2_w, p->fc2_b};
  return stlt_head(head, x, p->d, p->d, n, p->d, p->n_classes, p->ln_eps, h1, h2, logits, s);
}

// Token embedding + spatial transformer of the backbone (models.py:29-39,57-81) in the carved workspace.  *cls_rows / *cls_stride: where
// each frame's CLS row — the only row read afterwards (models.py:79) — lies: in x (stride N*d), or with STLT_FLAG_CLS_ONLY_LAST_SPATIAL
// compact in ctx.  x1 is free afterwards.  `o` applies to the layers that run whole (a sink goes with flags without CLS_ONLY).
static int spatial_tower(const stlt_params* p, const stlt_inputs* in, int flags, const WsBufs& w, const LayerOpts& o, const float** cls_rows_out,
                         int64_t* cls_stride_out, hipStream_t s) {
  const int64_t B = in->B, T = in->T, N = in->N, d = p->d, H = p->H;
  const int64_t tok = B * T * N, BT = B * T;
  float *x = w.x, *qkv = w.qkv, *ctx = w.ctx;
  // K1
  TRY(launch_embed(in->categories, in->boxes, in->scores, p->cat_emb, p->n_categories, p->box_w, p->box_b, p->score_w,
                   p->score_b, p->emb_ln_w, p->emb_ln_b, p->ln_eps, tok, d, x, s));
  // spatial transformer: sequences = frames (B*T), tokens = objects (N), key-padding mask only
  const bool cls_only = (flags & STLT_FLAG_CLS_ONLY_LAST_SPATIAL) && p->n_spatial > 0 && N > 1;
  const int64_t full_layers = cls_only ? p->n_spatial - 1 : p->n_spatial;
  for (int64_t l = 0; l < full_layers; ++l)
    TRY(encoder_layer(p->spatial[l], d, H, x, tok, BT, N, in->kpm_boxes, nullptr, nullptr, 0, STLT_K_ATTN_SPATIAL, qkv, ctx, w.tmp, w.x1, w.hh, x, s,
                      layer_opts(o, l, BT, N, H)));
  const float* cls_rows = x;
  int64_t cls_stride = N * d;
  if (cls_only) {
    // Only token 0 of each frame is read after the spatial transformer (models.py:79).  K and V are needed
    // for every object token, Q / out-proj / FFN only for the B*T CLS rows (rows of stride N*d in x).
    const stlt_layer_params& lp = p->spatial[p->n_spatial - 1];
    TRY(launch_linear(x, d, lp.in_proj_w + d * d, lp.in_proj_b + d, qkv + d, 3 * d, tok, 2 * d, d, STLT_ACT_NONE, s));
    TRY(launch_linear(x, N * d, lp.in_proj_w, lp.in_proj_b, qkv, N * 3 * d, BT, d, d, STLT_ACT_NONE, s));
    // non-CLS query rows of qkv hold stale scratch; each attention output row depends on its own query row
    // only, and only the CLS rows of ctx are read below.
    TRY(launch_attn(qkv, in->kpm_boxes, 0, BT, N, H, d / H, ctx, STLT_K_ATTN_SPATIAL, s));
    TRY(encoder_tail(lp, d, ctx, N * d, x, N * d, BT, false, w.tmp, w.x1, w.hh, ctx, s));  // compact CLS rows land in ctx's first BT rows
    cls_rows = ctx;
    cls_stride = d;
  }
  *cls_rows_out = cls_rows;
  *cls_stride_out = cls_stride;
  return 0;
}

// The first n_layers layers of the temporal transformer: sequences = clips (B), tokens = frames (T), causal + key padding.  Layers run in
// place on tbuf (a layer's input is last read by its norm1), x is the post-norm1 scratch; the tower's last layer writes `out`.
static int temporal_tower(const stlt_params* p, const stlt_inputs* in, int64_t n_layers, const WsBufs& w, const LayerOpts& o, float* tbuf, float* out,
                          hipStream_t s) {
  const int64_t B = in->B, T = in->T;
  for (int64_t l = 0; l < n_layers; ++l) {
    float* dst = (l == p->n_temporal - 1) ? out : tbuf;
    TRY(encoder_layer(p->temporal[l], p->d, p->H, tbuf, B * T, B, T, in->kpm_frames, nullptr, nullptr, 1, STLT_K_ATTN_TEMPORAL, w.qkv, w.ctx, w.tmp,
                      w.x, w.hh, dst, s, layer_opts(o, l, B, T, p->H)));
  }
  return 0;
}

// Backbone body in the carved workspace.  With last_rows != nullptr the final temporal layer only produces the rows the head reads
// (Stlt.forward, models.py:189-192: out[lengths-1, arange(B)]) into last_rows (B,d): K/V/Q are projected for every
// frame, the attention core runs as usual, but out-proj / norm1 / FFN / norm2 run on the B gathered rows only.
static int backbone_impl(const stlt_params* p, const stlt_inputs* in, const WsBufs& w, int flags, float* out_btd, float* last_rows, hipStream_t s) {
  const int64_t B = in->B, T = in->T, d = p->d;
  const float* cls_rows = nullptr;
  int64_t cls_stride = 0;
  TRY(spatial_tower(p, in, flags, w, LayerOpts{}, &cls_rows, &cls_stride, s));
  // K7: CLS select + position + frame type + LN -> (B,T,d).  x1 is free here (its last reader was the
  // final norm2 above), x / ctx still hold the CLS rows being read.
  float* tbuf = p->n_temporal > 0 ? w.x1 : out_btd;
  TRY(launch_frames_embed(cls_rows, cls_stride, in->frame_types, p->pos_emb, p->type_emb, p->frames_ln_w,
                          p->frames_ln_b, p->ln_eps, B, T, d, tbuf, s));
  TRY(temporal_tower(p, in, last_rows ? p->n_temporal - 1 : p->n_temporal, w, LayerOpts{}, tbuf, out_btd, s));
  if (last_rows) {
    const stlt_layer_params& lp = p->temporal[p->n_temporal - 1];
    float* g_ctx = w.x;                      // (B,d) gathered attention rows
    float* g_res = w.x + (size_t)B * d;      // (B,d) gathered layer-input rows (residual)
    float* g_x1 = w.hh + (size_t)B * 4 * d;  // (B,d) post-norm1, behind the (B,4d) FFN hidden (T > 1 => hh holds >= 2*B*4d)
    TRY(qkv_attention(lp, d, p->H, tbuf, B * T, B, T, in->kpm_frames, nullptr, nullptr, 1, STLT_K_ATTN_TEMPORAL, w.qkv, w.ctx, s));
    TRY(launch_gather_last(w.ctx, in->lengths, B, T, d, g_ctx, s));
    TRY(launch_gather_last(tbuf, in->lengths, B, T, d, g_res, s));
    TRY(encoder_tail(lp, d, g_ctx, d, g_res, d, B, false, w.tmp, g_x1, w.hh, last_rows, s));
  }
  return 0;
}

// The tail of an encoder layer (out-proj, norm1, FFN, norm2) on n rows picked out of the layer's attention output
// and input: what the layer computes for rows whose output is the only thing read afterwards.
static int encoder_tail_rows(const stlt_layer_params& lp, int64_t d, const float* ctx, const float* x, const int* rows, int64_t n,
                             float* g_ctx, float* g_res, float* g_x1, float* tmp, float* hh, float* out, hipStream_t s) {
  TRY(launch_gather_rows(ctx, d, rows, n, d, g_ctx, s));
  TRY(launch_gather_rows(x, d, rows, n, d, g_res, s));
  return encoder_tail(lp, d, g_ctx, d, g_res, d, n, false, tmp, g_x1, hh, out, s);
}

// Stlt.forward up to the rows the head reads, computed on the real tokens / frames only (STLT_FLAG_SKIP_PADDING).
// Synchronises the stream once, to read the two row counts the launches are sized by.
// out_btd != null (the fusion models' layout branch): every temporal layer runs on all real frames and the result is
// scattered into the (B,T,d) tensor, padded frames zero — those rows are only ever masked keys or queries whose outputs
// nobody reads (models.py:403-431, 470), so the logits are the padded schedule's; h0 is not produced.
static int forward_ragged(const stlt_params* p, const stlt_inputs* in, const WsBufs& w, float* h0, float* out_btd, hipStream_t s) {
  const int64_t B = in->B, T = in->T, N = in->N, d = p->d, H = p->H;
  // head dims other than 64 run the ragged attention on attn_any.hip, whose forward holds at most 1024 keys of a segment (a frame's N
  // slots, a clip's T frames) in LDS: longer segments are refused here instead of being truncated in the kernel
  if (d / H != 64 && (N > 1024 || T > 1024))
    return stlt_set_error(STLT_EINVAL, "skip-padding with head dim %lld (not 64) takes at most 1024 object slots / frames per segment (N=%lld, T=%lld)", (long long)(d / H), (long long)N, (long long)T);
  float *x = w.x, *x1 = w.x1, *qkv = w.qkv, *ctx = w.ctx, *tmp = w.tmp, *hh = w.hh;
  const RaggedIndex ix = ragged_index_carve(w.ridx, B, T, N);
  TRY(launch_ragged_index(in->kpm_boxes, in->kpm_frames, in->lengths, B, T, N, ix, s));
  int64_t Ms = 0, Mf = 0;
  bool host_counts = false;  // the caller knows the two row counts: no read-back, no synchronisation
  TRY(read_ragged_counts(ix, in, true, Ms, Mf, &host_counts, s));
  TRY(launch_embed(in->categories, in->boxes, in->scores, p->cat_emb, p->n_categories, p->box_w, p->box_b, p->score_w,
                   p->score_b, p->emb_ln_w, p->emb_ln_b, p->ln_eps, Ms, d, x, s, nullptr, StltDrop{0u, 1.0f, 0ull}, ix.t_orig));
  // spatial transformer: segments = frames; after it only each frame's CLS row is read (models.py:79)
  for (int64_t l = 0; l + 1 < p->n_spatial; ++l)
    TRY(encoder_layer(p->spatial[l], d, H, x, Ms, 0, 0, nullptr, ix.t_seg_start, ix.t_seg_end, 0, STLT_K_ATTN_SPATIAL, qkv, ctx, tmp, x1, hh, x, s));
  float* cls = ctx;  // (Mf, d)
  if (p->n_spatial > 0) {
    const stlt_layer_params& lp = p->spatial[p->n_spatial - 1];
    TRY(qkv_attention(lp, d, H, x, Ms, 0, 0, nullptr, ix.t_seg_start, ix.t_seg_end, 0, STLT_K_ATTN_SPATIAL, qkv, ctx, s));
    // qkv is dead once ctx exists: it holds the gathered rows; the layer output lands in ctx's first Mf rows
    // (ctx rows are read by the gather before anything is written back)
    TRY(encoder_tail_rows(lp, d, ctx, x, ix.f_cls_row, Mf, qkv, qkv + (size_t)Mf * d, x1, tmp, hh, qkv + (size_t)2 * Mf * d, s));
    cls = qkv + (size_t)2 * Mf * d;
  } else {
    TRY(launch_gather_rows(x, d, ix.f_cls_row, Mf, d, ctx, s));
  }
  // frames embedding on the real frames (position / frame type looked up through the frame's place in the padded batch)
  float* tbuf = x1;
  TRY(launch_frames_embed(cls, d, in->frame_types, p->pos_emb, p->type_emb, p->frames_ln_w, p->frames_ln_b, p->ln_eps, B, T,
                          d, tbuf, s, nullptr, StltDrop{0u, 1.0f, 0ull}, ix.f_orig, Mf));
  // temporal transformer: segments = clips, causal
  const int64_t tp_full = out_btd ? p->n_temporal : p->n_temporal - 1;
  for (int64_t l = 0; l < tp_full; ++l)
    TRY(encoder_layer(p->temporal[l], d, H, tbuf, Mf, 0, 0, nullptr, ix.f_seg_start, ix.f_seg_end, 1, STLT_K_ATTN_TEMPORAL, qkv, ctx, tmp, x, hh, tbuf, s));
  if (out_btd) {
    TRY(launch_scatter_rows(tbuf, ix.f_orig, Mf, d, out_btd, B * T, s, host_counts ? ix.counts + 1 : nullptr));
    return host_counts ? launch_ragged_poison(ix, Ms, Mf, true, out_btd, B * T * d, s) : 0;
  }
  if (p->n_temporal > 0) {
    const stlt_layer_params& lp = p->temporal[p->n_temporal - 1];
    TRY(qkv_attention(lp, d, H, tbuf, Mf, 0, 0, nullptr, ix.f_seg_start, ix.f_seg_end, 1, STLT_K_ATTN_TEMPORAL, qkv, ctx, s));
    TRY(encoder_tail_rows(lp, d, ctx, tbuf, ix.last_row, B, x, qkv, qkv + (size_t)B * d, tmp, hh, h0, s));  // qkv is dead once ctx exists
  } else {
    TRY(launch_gather_rows(tbuf, d, ix.last_row, B, d, h0, s));
  }
  // the caller's counts were taken on trust; in inference they may be upper bounds (the rows in between are dummies nobody reads).  Real counts
  // above them, or masks that break the contract: NaN rows for the head, NaN logits
  return host_counts ? launch_ragged_poison(ix, Ms, Mf, true, h0, B * d, s) : 0;
}

// for caf.hip (declared in common.h)
int backbone_impl_public(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes, int flags,
                         float* out_btd, hipStream_t s) {
  TRY(check_params(p, in, false));
  WsBufs w;
  TRY(ws_carve(p, in, 1, workspace, workspace_bytes, STLT_EWORKSPACE, "", &w));
  StltGemmScratch gemm_scratch(w.sk, STLT_GEMM_SCRATCH_BYTES);
  if (flags & STLT_FLAG_SKIP_PADDING) {
    if (!out_btd) return stlt_set_error(STLT_EINVAL, "skip-padding backbone: out_btd is null");
    return forward_ragged(p, in, w, nullptr, out_btd, s);
  }
  return backbone_impl(p, in, w, flags, out_btd, nullptr, s);
}

// for caf.hip (declared in common.h): the towers of stlt_forward_attention, the (B,T,d) state instead of the head
int backbone_attention_public(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes, int per_head,
                              float* attn_spatial, float* attn_temporal, float* out_btd, hipStream_t s) {
  TRY(check_params(p, in, false));
  if (!out_btd) return stlt_set_error(STLT_EINVAL, "attention backbone: out_btd is null");
  WsBufs w;
  TRY(ws_carve(p, in, 1, workspace, workspace_bytes, STLT_EWORKSPACE, "", &w));
  StltGemmScratch gemm_scratch(w.sk, STLT_GEMM_SCRATCH_BYTES);
  const float* cls_rows = nullptr;
  int64_t cls_stride = 0;
  TRY(spatial_tower(p, in, 0, w, LayerOpts{true, attn_spatial, per_head}, &cls_rows, &cls_stride, s));
  float* tbuf = p->n_temporal > 0 ? w.x1 : out_btd;  // x1 is free: its last reader was the final norm2 above
  TRY(launch_frames_embed(cls_rows, cls_stride, in->frame_types, p->pos_emb, p->type_emb, p->frames_ln_w, p->frames_ln_b, p->ln_eps, in->B, in->T, p->d,
                          tbuf, s));
  return temporal_tower(p, in, p->n_temporal, w, LayerOpts{true, attn_temporal, per_head}, tbuf, out_btd, s);
}

extern "C" {

size_t stlt_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_classes) {
  if (B <= 0 || T <= 0 || N <= 0 || d <= 0) return 0;
  return stlt_ws_bytes(B, T, N, d, n_classes, 1);
}

size_t stlt_prefix_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_classes) {
  if (B <= 0 || T <= 0 || N <= 0 || d <= 0) return 0;
  return stlt_ws_bytes(B, T, N, d, n_classes, 2);
}

size_t stlt_attention_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t n_classes) {
  if (B <= 0 || T <= 0 || N <= 0 || d <= 0) return 0;
  return stlt_ws_bytes(B, T, N, d, n_classes, 1);
}

int stlt_backbone_forward(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes,
                          int flags, float* out_btd, stlt_stream_t stream) {
  TRY(check_params(p, in, false));
  if (!out_btd) return stlt_set_error(STLT_EINVAL, "stlt_backbone_forward: out_btd is null");
  WsBufs w;
  TRY(ws_carve(p, in, 1, workspace, workspace_bytes, STLT_EWORKSPACE, "", &w));
  StltGemmScratch gemm_scratch(w.sk, STLT_GEMM_SCRATCH_BYTES);
  return backbone_impl(p, in, w, flags, out_btd, nullptr, (hipStream_t)stream);
}

int stlt_forward(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes, int flags,
                 float* out_btd, float* logits, stlt_stream_t stream) {
  TRY(check_params(p, in, true));
  if (!logits) return stlt_set_error(STLT_EINVAL, "stlt_forward: logits is null");
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = in->B, T = in->T, d = p->d;
  WsBufs w;
  TRY(ws_carve(p, in, 1, workspace, workspace_bytes, STLT_EWORKSPACE, "", &w));
  StltGemmScratch gemm_scratch(w.sk, STLT_GEMM_SCRATCH_BYTES);
  float* bb_out = out_btd ? out_btd : w.x1;  // x1 doubles as the in-place temporal buffer
  float* h0 = w.head;
  const bool last_only = (flags & STLT_FLAG_LAST_ROW_ONLY_TEMPORAL) && !out_btd && p->n_temporal > 0 && in->T > 1;
  if ((flags & STLT_FLAG_SKIP_PADDING) && !out_btd) {  // padded rows are never computed, so there is no (B,T,d) output to hand back
    TRY(forward_ragged(p, in, w, h0, nullptr, s));
  } else if (last_only) {  // the caller does not want the (B,T,d) backbone output: produce only the rows the head reads
    TRY(backbone_impl(p, in, w, flags, bb_out, h0, s));
  } else {
    TRY(backbone_impl(p, in, w, flags, bb_out, nullptr, s));
    TRY(launch_gather_last(bb_out, in->lengths, B, T, d, h0, s));                                 // models.py:189-192
  }
  return classification_head(p, h0, B, h0 + (size_t)B * d, h0 + (size_t)2 * B * d, logits, s);
}

int stlt_attn_prefix_probe_fwd(const float* qkv_frames, const float* qkv_probes, const uint8_t* kpm, int64_t S, int64_t T, int64_t H, int64_t dh,
                               float* ctx, stlt_stream_t stream) {
  return launch_attn_prefix_probe(qkv_frames, qkv_probes, kpm, S, T, H, dh, ctx, (hipStream_t)stream);
}

// Two temporal streams stacked as one (2*B*T, d) matrix: rows [0, B*T) the frames, rows [B*T, 2*B*T) the probes (probe (b,t): the clip's
// extract frame at position t).  Every product and LayerNorm of a layer is one launch over both; the frames run the ordinary causal
// attention, the probes launch_attn_prefix_probe.  In the last layer the frames are needed as keys and values only.
int stlt_forward_prefixes(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes, int flags, float* logits,
                          stlt_stream_t stream) {
  TRY(check_params(p, in, true));
  if (!logits) return stlt_set_error(STLT_EINVAL, "stlt_forward_prefixes: logits is null");
  if (flags & STLT_FLAG_SKIP_PADDING)
    return stlt_set_error(STLT_EINVAL, "stlt_forward_prefixes: STLT_FLAG_SKIP_PADDING is not supported (the per-prefix forward runs the padded schedule)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = in->B, T = in->T, d = p->d, H = p->H, BT = B * T;
  WsBufs w;
  TRY(ws_carve(p, in, 2, workspace, workspace_bytes, STLT_EWORKSPACE, "", &w));
  StltGemmScratch gemm_scratch(w.sk, STLT_GEMM_SCRATCH_BYTES);
  float *x = w.x, *qkv = w.qkv, *ctx = w.ctx, *tmp = w.tmp, *hh = w.hh;
  const float* cls_rows = nullptr;
  int64_t cls_stride = 0;
  TRY(spatial_tower(p, in, flags, w, LayerOpts{}, &cls_rows, &cls_stride, s));
  // both streams' embeddings into x1 (free here; x / ctx still hold the CLS rows being read)
  float* g = w.x1;                      // frames (BT,d)
  float* pr = w.x1 + (size_t)BT * d;    // probes (BT,d)
  TRY(launch_frames_embed(cls_rows, cls_stride, in->frame_types, p->pos_emb, p->type_emb, p->frames_ln_w, p->frames_ln_b, p->ln_eps, B, T, d, g, s));
  TRY(launch_probes_embed(cls_rows, cls_stride, in->frame_types, in->lengths, p->pos_emb, p->type_emb, p->frames_ln_w, p->frames_ln_b, p->ln_eps, B, T,
                          d, pr, s));
  float* qkv_p = qkv + (size_t)BT * 3 * d;
  float* ctx_p = ctx + (size_t)BT * d;
  for (int64_t l = 0; l < p->n_temporal; ++l) {
    const stlt_layer_params& lp = p->temporal[l];
    if (l + 1 < p->n_temporal) {
      TRY(launch_linear(g, d, lp.in_proj_w, lp.in_proj_b, qkv, 3 * d, 2 * BT, 3 * d, d, STLT_ACT_NONE, s));
      TRY(launch_attn(qkv, in->kpm_frames, 1, B, T, H, d / H, ctx, STLT_K_ATTN_TEMPORAL, s));
      TRY(launch_attn_prefix_probe(qkv, qkv_p, in->kpm_frames, B, T, H, d / H, ctx_p, s));
      TRY(encoder_tail(lp, d, ctx, d, g, d, 2 * BT, fuse_residual(), tmp, x, hh, g, s));  // in place, as the backbone's temporal layers
    } else {
      // the frames' query columns of qkv keep stale scratch: the probe attention reads their keys and values only
      TRY(launch_linear(g, d, lp.in_proj_w + d * d, lp.in_proj_b + d, qkv + d, 3 * d, BT, 2 * d, d, STLT_ACT_NONE, s));
      TRY(launch_linear(pr, d, lp.in_proj_w, lp.in_proj_b, qkv_p, 3 * d, BT, 3 * d, d, STLT_ACT_NONE, s));
      TRY(launch_attn_prefix_probe(qkv, qkv_p, in->kpm_frames, B, T, H, d / H, ctx_p, s));
      TRY(encoder_tail(lp, d, ctx_p, d, pr, d, BT, fuse_residual(), tmp, x, hh, pr, s));
    }
  }
  // the head on the B*T probe rows; qkv and ctx are dead: they hold its two (BT,d) intermediates
  TRY(classification_head(p, pr, BT, qkv, ctx, logits, s));
  return launch_prefix_zero_invalid(logits, in->lengths, B, T, p->n_classes, s);
}

int stlt_attn_probs_fwd(const float* qkv, const uint8_t* kpm, int causal, int64_t S, int64_t L, int64_t H, int64_t dh, int per_head, float* probs,
                        stlt_stream_t stream) {
  return launch_attn_probs(qkv, kpm, causal, S, L, H, dh, per_head, probs, (hipStream_t)stream);
}

int stlt_attn_probs_cross_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const uint8_t* kpm, int causal, int64_t S, int64_t Lq,
                              int64_t Lk, int64_t H, int64_t dh, int per_head, float* probs, stlt_stream_t stream) {
  return launch_attn_probs_cross(q, ldq, k, ldk, kpm, causal, S, Lq, Lk, H, dh, per_head, probs, (hipStream_t)stream);
}

// The dense schedule with every layer as the unfused pair, maps or no maps: the layer's packed QKV lies in the workspace, and the attention
// core and the probabilities launch read it side by side.
int stlt_forward_attention(const stlt_params* p, const stlt_inputs* in, void* workspace, size_t workspace_bytes, int flags, int per_head, float* logits,
                           float* attn_spatial, float* attn_temporal, stlt_stream_t stream) {
  TRY(check_params(p, in, true));
  if (!logits) return stlt_set_error(STLT_EINVAL, "stlt_forward_attention: logits is null");
  if (flags & STLT_FLAG_SKIP_PADDING)
    return stlt_set_error(STLT_EINVAL, "stlt_forward_attention: STLT_FLAG_SKIP_PADDING is not supported (the attention maps are those of the padded schedule)");
  if (per_head != 0 && per_head != 1) return stlt_set_error(STLT_EINVAL, "stlt_forward_attention: per_head must be 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = in->B, T = in->T, N = in->N, d = p->d;
  if ((attn_spatial && p->n_spatial > 0 && N > 1024) || (attn_temporal && p->n_temporal > 0 && T > 1024))
    return stlt_set_error(STLT_EINVAL, "stlt_forward_attention: a map of more than 1024 keys (N=%lld, T=%lld)", (long long)N, (long long)T);
  if (((uintptr_t)logits | (uintptr_t)attn_spatial | (uintptr_t)attn_temporal) & 3)
    return stlt_set_error(STLT_EINVAL, "stlt_forward_attention: logits / attn_spatial / attn_temporal must be 4-byte aligned");
  WsBufs w;
  TRY(ws_carve(p, in, 1, workspace, workspace_bytes, STLT_EINVAL, "stlt_forward_attention: ", &w));
  StltGemmScratch gemm_scratch(w.sk, STLT_GEMM_SCRATCH_BYTES);
  const float* cls_rows = nullptr;
  int64_t cls_stride = 0;
  TRY(spatial_tower(p, in, 0, w, LayerOpts{true, attn_spatial, per_head}, &cls_rows, &cls_stride, s));  // the elision flags do not apply: every row of every map is asked for
  float* tbuf = w.x1;  // free: its last reader was the final norm2 above
  TRY(launch_frames_embed(cls_rows, cls_stride, in->frame_types, p->pos_emb, p->type_emb, p->frames_ln_w, p->frames_ln_b, p->ln_eps, B, T, d, tbuf, s));
  TRY(temporal_tower(p, in, p->n_temporal, w, LayerOpts{true, attn_temporal, per_head}, tbuf, tbuf, s));
  float* h0 = w.head;
  TRY(launch_gather_last(tbuf, in->lengths, B, T, d, h0, s));  // models.py:189-192
  return classification_head(p, h0, B, h0 + (size_t)B * d, h0 + (size_t)2 * B * d, logits, s);
}

}  // extern "C"
