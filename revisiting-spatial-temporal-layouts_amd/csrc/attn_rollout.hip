// Attention rollout and relevance read-out (include/stlt_hip.h: stlt_attn_rollout, stlt_relevance_combine, stlt_attn_rollout_joint,
// stlt_relevance_combine_joint): what turns the gradient-weighted attention maps of attn_grad_probs.hip into the per-object relevance of a
// prediction (Chefer, Gur, Wolf 2021) — for one tower, and for the fusion models, whose residual stream runs over two modalities that attend
// to each other (CrossModalModule, reference models.py:403-431).  The reference has none of this.  The C entry points of the grad-probs
// launchers sit here too, beside those of the rollouts they feed.
//
//   rollout:    R_0 = I, R_l = R_{l-1} + abar_l · R_{l-1}.  The columns of R never mix (column j of R_l depends on column j of R_{l-1} alone), so
//               a workgroup keeps a block of columns of one item's R in LDS, ping-pong, for the WHOLE chain while the layers stream in from
//               memory: one launch whatever the length.  L <= 64: the block is every column, and several items share a workgroup when L is small;
//               64 < L <= 256: blocks of 16 columns, (L, 16) floats a side.  fp32 FMA over k in ascending order from zero, R_{l-1}[i,j] added last.
//   combine:    rel[b,t,n] = R_temporal[b, lengths[b]-1, t] * R_spatial[b,t,0,n]  (row 0 of a frame is its CLS token, models.py:79; the head
//               reads frame lengths-1 of a clip, models.py:189-192).
//   joint rollout: R over the J = T + A stacked tokens, R_0 = blockdiag(r_layout, r_appearance), then per fusion layer three steps R <- R + X·R with
//               X = [[0, l2a], [a2l, 0]], blockdiag(f_layout, f_appearance[.,0]), blockdiag(0, f_appearance[.,1]).  Only the non-zero quadrants are
//               read.  The columns of R never mix, so a workgroup keeps 16 columns of one item's R in LDS, ping-pong, for the whole chain: one
//               launch; 2 x 512 x 16 floats = 64 KB at the largest J.  fp32 FMA over k in ascending order from zero, the old R[i,j] added last.
//   joint combine: row[b,:] = w_layout R[b, lengths[b]-1, :] + w_appearance R[b, T, :] (the frame the layout head reads, models.py:189-192, and the
//               appearance CLS token, models.py:260-262); frame_rel = row[:T], app_rel = row[T:], rel[b,t,n] = frame_rel[b,t] * r_spatial[b,t,0,n].
#include <cstdint>
#include "common.h"

namespace {

constexpr int RO_MAX_L = 256;  // the grad-probs launchers' own limit (the attention backward's domain, backward.hip)

// ---- rollout ---------------------------------------------------------------------------------------------------------------------------
constexpr int RO_THREADS = 256;
constexpr int RO_TILE = 4096;   // floats of R a workgroup holds per side: (L, CB) x P items
constexpr int RO_COLS = 16;     // column block above 64 tokens

struct RolloutGeo {
  const float* abar;  // (n_layers, S, L, L)
  float* R;           // (S, L, L)
  int64_t S;
  int n_layers, L, CB, P, NCB;  // CB columns per block, P items per workgroup, NCB column blocks per item
};

__global__ __launch_bounds__(RO_THREADS) void attn_rollout_kernel(const RolloutGeo geo) {
  __shared__ float r_lds[2][RO_TILE];
  const int L = geo.L, CB = geo.CB, P = geo.P;
  const int tile = L * CB;                  // floats of one item's block
  const int64_t grp = blockIdx.x / geo.NCB;   // group of P items
  const int jb = (int)(blockIdx.x - grp * geo.NCB);
  const int64_t map = (int64_t)L * L;
  const int n_el = P * tile;                // <= RO_TILE
  // R_0 = I
  for (int e = threadIdx.x; e < n_el; e += RO_THREADS) {
    const int rem = e % tile;
    const int i = rem / CB, j = rem - i * CB;
    r_lds[0][e] = i == jb * CB + j ? 1.f : 0.f;
  }
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < geo.n_layers; ++l) {
    const float* old = r_lds[cur];
    float* nxt = r_lds[cur ^ 1];
    for (int e = threadIdx.x; e < n_el; e += RO_THREADS) {
      const int p = e / tile, rem = e - p * tile;
      const int i = rem / CB, j = rem - i * CB;
      const int64_t item = grp * P + p;
      float a = 0.f;  // the chain starts from zero and the old value joins it once, last: started from old[e], every one of the L products
                      // rounds at R's magnitude — 45 u on the diagonal of a map of scale 1e-2, where R = 1 + 1e-2 (profiles/explain_scale.md)
      if (item < geo.S) {  // (the items past the end keep their identity and are never stored)
        const float* arow = geo.abar + ((int64_t)l * geo.S + item) * map + (int64_t)i * L;
        const float* col = old + p * tile + j;
        for (int k = 0; k < L; ++k) a = fmaf(arow[k], col[k * CB], a);
      }
      nxt[e] = old[e] + a;
    }
    __syncthreads();
    cur ^= 1;
  }
  for (int e = threadIdx.x; e < n_el; e += RO_THREADS) {
    const int p = e / tile, rem = e - p * tile;
    const int i = rem / CB, j = rem - i * CB;
    const int64_t item = grp * P + p;
    const int jc = jb * CB + j;
    if (item < geo.S && jc < L) geo.R[item * map + (int64_t)i * L + jc] = r_lds[cur][e];
  }
}

// ---- combine ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relevance_combine_kernel(const float* __restrict__ rt, const float* __restrict__ rs, const int64_t* __restrict__ lengths,
                                                               int64_t B, int64_t T, int64_t N, float* __restrict__ rel) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= B * T * N) return;
  const int64_t f = e / N, n = e - f * N;  // frame b*T + t, object slot
  const int64_t b = f / T, t = f - b * T;
  const int64_t len = lengths[b];
  // a length outside 1 ... T names no read-out row: NaN, the convention of stlt_loss_fwd_bwd for an out-of-range label
  rel[e] = len >= 1 && len <= T ? rt[(b * T + len - 1) * T + t] * rs[f * N * N + n] : __builtin_nanf("");
}

// ---- joint rollout -----------------------------------------------------------------------------------------------------------------------
constexpr int JR_THREADS = 256;
constexpr int JR_COLS = 16;               // columns of R a workgroup carries through the chain
constexpr int JR_MAX_J = 2 * RO_MAX_L;    // T, A <= 256
constexpr int JR_TILE = JR_MAX_J * JR_COLS;  // floats a side: 2 x 32 KB of static LDS

struct JointGeo {
  const float* r_layout;      // (S, T, T) or NULL = identity
  const float* r_appearance;  // (S, A, A) or NULL = identity
  const float* l2a;           // (n, S, T, A)
  const float* a2l;           // (n, S, A, T)
  const float* f_layout;      // (n, S, T, T)
  const float* f_appearance;  // (n, 2, S, A, A)
  float* R;                   // (S, J, J)
  int64_t S;
  int n_fusion, T, A, CB, NCB;  // CB columns per block, NCB column blocks per item
};

__global__ __launch_bounds__(JR_THREADS) void attn_rollout_joint_kernel(const JointGeo geo) {
  __shared__ float r_lds[2][JR_TILE];
  const int T = geo.T, A = geo.A, J = T + A, CB = geo.CB;
  const int64_t item = blockIdx.x / geo.NCB;
  const int jb = (int)(blockIdx.x - item * geo.NCB);
  const int tile = J * CB;  // <= JR_TILE
  const int64_t S = geo.S;
  // R_0 = blockdiag(r_layout, r_appearance); the columns past J of the last block are zeros and are never stored
  for (int e = threadIdx.x; e < tile; e += JR_THREADS) {
    const int i = e / CB, jc = jb * CB + (e - i * CB);
    float r0 = 0.f;
    if (i < T && jc < T) r0 = geo.r_layout ? geo.r_layout[(item * T + i) * T + jc] : (i == jc ? 1.f : 0.f);
    else if (i >= T && jc >= T && jc < J) r0 = geo.r_appearance ? geo.r_appearance[(item * A + (i - T)) * A + (jc - T)] : (i == jc ? 1.f : 0.f);
    r_lds[0][e] = r0;
  }
  __syncthreads();
  int cur = 0;
  // one step R <- R + X·R: the layout rows of X are map_t (T, n_t) over the joint tokens k0_t .. k0_t + n_t - 1 (NULL: a zero row block), the
  // appearance rows map_a (A, n_a) over k0_a .. k0_a + n_a - 1
  auto step = [&](const float* map_t, int k0_t, int n_t, const float* map_a, int k0_a, int n_a) __attribute__((always_inline)) {
    const float* old = r_lds[cur];
    float* nxt = r_lds[cur ^ 1];
    for (int e = threadIdx.x; e < tile; e += JR_THREADS) {
      const int i = e / CB, j = e - i * CB;
      float a = 0.f;  // from zero, the old value added last: see attn_rollout_kernel
      const bool top = i < T;
      const float* arow = top ? (map_t ? map_t + (int64_t)i * n_t : nullptr) : map_a + (int64_t)(i - T) * n_a;
      if (arow) {
        const int n = top ? n_t : n_a;
        const float* col = old + (top ? k0_t : k0_a) * CB + j;
        for (int k = 0; k < n; ++k) a = fmaf(arow[k], col[k * CB], a);
      }
      nxt[e] = old[e] + a;
    }
    __syncthreads();
    cur ^= 1;
  };
  const int64_t ta = (int64_t)T * A, tt = (int64_t)T * T, aa = (int64_t)A * A;
  for (int l = 0; l < geo.n_fusion; ++l) {
    step(geo.l2a + (l * S + item) * ta, T, A, geo.a2l + (l * S + item) * ta, 0, T);
    step(geo.f_layout + (l * S + item) * tt, 0, T, geo.f_appearance + ((2 * l) * S + item) * aa, T, A);
    step(nullptr, 0, 0, geo.f_appearance + ((2 * l + 1) * S + item) * aa, T, A);
  }
  for (int e = threadIdx.x; e < tile; e += JR_THREADS) {
    const int i = e / CB, jc = jb * CB + (e - i * CB);
    if (jc < J) geo.R[(item * J + i) * J + jc] = r_lds[cur][e];
  }
}

// ---- joint combine -----------------------------------------------------------------------------------------------------------------------
struct CombineGeo {
  const float* R;          // (B, J, J)
  const float* r_spatial;  // (B*T, N, N)
  const int64_t* lengths;  // (B)
  float *rel, *frame_rel, *app_rel;  // (B, T, N), (B, T), (B, A)
  int64_t B, T, A, N;
  float w_layout, w_appearance;
};

__global__ __launch_bounds__(256) void relevance_combine_joint_kernel(const CombineGeo geo) {
  const int64_t T = geo.T, A = geo.A, N = geo.N, J = T + A;
  const int64_t per_clip = T * N + J;  // rel, then frame_rel, then app_rel
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= geo.B * per_clip) return;
  const int64_t b = e / per_clip, r = e - b * per_clip;
  const int64_t j = r < T * N ? r / N : r - T * N;  // the joint token whose entry of the read-out row this element needs
  const int64_t len = geo.lengths[b];
  // a length outside 1 ... T names no read-out row: NaN, the convention of stlt_relevance_combine
  float row = __builtin_nanf("");
  if (len >= 1 && len <= T) {
    const float* Rb = geo.R + b * J * J;
    row = (geo.w_layout != 0.f ? geo.w_layout * Rb[(len - 1) * J + j] : 0.f) + (geo.w_appearance != 0.f ? geo.w_appearance * Rb[T * J + j] : 0.f);
  }
  if (r < T * N) {
    const int64_t n = r - j * N;
    geo.rel[(b * T + j) * N + n] = row * geo.r_spatial[(b * T + j) * N * N + n];
  } else if (j < T) {
    geo.frame_rel[b * T + j] = row;
  } else {
    geo.app_rel[b * A + (j - T)] = row;
  }
}

}  // namespace

int launch_attn_rollout(const float* abar, int64_t n_layers, int64_t S, int64_t L, float* R, hipStream_t s) {
  if (!R || (n_layers > 0 && !abar)) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: null pointer");
  if (n_layers < 0 || n_layers > 64) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: layer count %lld unsupported (0 ... 64)", (long long)n_layers);
  if (L < 1 || L > RO_MAX_L) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: sequence length %lld unsupported (1 ... %d)", (long long)L, RO_MAX_L);
  if (S < 0 || S > 0x7fffff00LL || S * L > 0x7fffff00LL) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: bad sequence count");
  if ((uintptr_t)abar & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: abar must be 4-byte aligned");
  if ((uintptr_t)R & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: R must be 4-byte aligned");
  if (S == 0) return 0;
  RolloutGeo g;
  g.abar = abar; g.R = R; g.S = S; g.n_layers = (int)n_layers; g.L = (int)L;
  if (L <= 64) {
    g.CB = (int)L; g.NCB = 1;
    g.P = (int)(RO_TILE / (L * L));  // >= 1
    if (g.P > 64) g.P = 64;
    if (g.P > S) g.P = (int)S;
  } else {
    g.CB = RO_COLS; g.NCB = (int)((L + RO_COLS - 1) / RO_COLS); g.P = 1;  // L * 16 <= RO_TILE
  }
  const int64_t n_wg = (S + g.P - 1) / g.P * g.NCB;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: too many work items");
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("attn_rollout layers=%lld S=%lld L=%lld items/wg=%d cols/wg=%d", (long long)n_layers, (long long)S, (long long)L, g.P, g.CB);
  stlt_prof_add_bytes((double)(n_layers * g.NCB + 1) * S * L * L * 4.0);
  stlt_prof_note_flops((double)n_layers * S * L * L * L * 2.0);
  hipLaunchKernelGGL(attn_rollout_kernel, dim3((unsigned)n_wg), dim3(RO_THREADS), 0, s, g);
  return stlt_check_launch("attn_rollout_kernel");
}

int launch_relevance_combine(const float* r_temporal, const float* r_spatial, const int64_t* lengths, int64_t B, int64_t T, int64_t N, float* rel, hipStream_t s) {
  if (!r_temporal || !r_spatial || !lengths || !rel) return stlt_set_error(STLT_EINVAL, "stlt_relevance_combine: null pointer");
  if (B < 0 || T < 1 || N < 1 || T > 0x7fffLL || N > 0x7fffLL || B > 0x7fffff00LL || B * T * N > 0x7fffff00LL)
    return stlt_set_error(STLT_EINVAL, "stlt_relevance_combine: bad batch shape");
  for (const StltNamedPtr& q : {StltNamedPtr{"r_temporal", r_temporal}, StltNamedPtr{"r_spatial", r_spatial}, StltNamedPtr{"rel", rel}})
    if ((uintptr_t)q.p & 3) return stlt_set_error(STLT_EINVAL, "stlt_relevance_combine: %s must be 4-byte aligned", q.name);
  if ((uintptr_t)lengths & 7) return stlt_set_error(STLT_EINVAL, "stlt_relevance_combine: lengths must be 8-byte aligned");
  if (B == 0) return 0;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("relevance_combine B=%lld T=%lld N=%lld", (long long)B, (long long)T, (long long)N);
  stlt_prof_add_bytes((double)B * T * N * 4.0 * 2 + (double)B * T * 4.0);
  hipLaunchKernelGGL(relevance_combine_kernel, dim3((unsigned)((B * T * N + 255) / 256)), dim3(256), 0, s, r_temporal, r_spatial, lengths, B, T, N, rel);
  return stlt_check_launch("relevance_combine_kernel");
}

int launch_attn_rollout_joint(const float* r_layout, const float* r_appearance, const float* l2a, const float* a2l, const float* f_layout, const float* f_appearance,
                              int64_t n_fusion, int64_t S, int64_t T, int64_t A, float* R, hipStream_t s) {
  if (!R || (n_fusion > 0 && (!l2a || !a2l || !f_layout || !f_appearance))) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: null pointer");
  if (n_fusion < 0 || n_fusion > 64) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: layer count %lld unsupported (0 ... 64)", (long long)n_fusion);
  if (T < 1 || T > RO_MAX_L || A < 1 || A > RO_MAX_L)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: token counts %lld / %lld unsupported (1 ... %d)", (long long)T, (long long)A, RO_MAX_L);
  const int64_t J = T + A;
  if (S < 0 || S > 0x7fffff00LL || S * J > 0x7fffff00LL) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: bad sequence count");
  for (const StltNamedPtr& q : {StltNamedPtr{"r_layout", r_layout}, StltNamedPtr{"r_appearance", r_appearance}, StltNamedPtr{"layout_to_appearance", l2a},
                                StltNamedPtr{"appearance_to_layout", a2l}, StltNamedPtr{"fusion_layout", f_layout}, StltNamedPtr{"fusion_appearance", f_appearance},
                                StltNamedPtr{"R", R}})
    if ((uintptr_t)q.p & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: %s must be 4-byte aligned", q.name);
  if (S == 0) return 0;
  JointGeo g;
  g.r_layout = r_layout; g.r_appearance = r_appearance; g.l2a = l2a; g.a2l = a2l; g.f_layout = f_layout; g.f_appearance = f_appearance; g.R = R;
  g.S = S; g.n_fusion = (int)n_fusion; g.T = (int)T; g.A = (int)A;
  g.CB = J < JR_COLS ? (int)J : JR_COLS;  // J * CB <= JR_TILE
  g.NCB = (int)((J + g.CB - 1) / g.CB);
  const int64_t n_wg = S * g.NCB;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: too many work items");
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("attn_rollout_joint layers=%lld S=%lld T=%lld A=%lld cols/wg=%d", (long long)n_fusion, (long long)S, (long long)T, (long long)A, g.CB);
  stlt_prof_add_bytes(((double)n_fusion * g.NCB * (2.0 * T * A + T * T + 2.0 * A * A) + (double)T * T + (double)A * A + (double)J * J) * S * 4.0);
  stlt_prof_note_flops((double)n_fusion * S * J * (2.0 * T * A + T * T + 2.0 * A * A) * 2.0);
  hipLaunchKernelGGL(attn_rollout_joint_kernel, dim3((unsigned)n_wg), dim3(JR_THREADS), 0, s, g);
  return stlt_check_launch("attn_rollout_joint_kernel");
}

int launch_relevance_combine_joint(const float* R, const float* r_spatial, const int64_t* lengths, int64_t B, int64_t T, int64_t A, int64_t N, float w_layout,
                                   float w_appearance, float* rel, float* frame_rel, float* app_rel, hipStream_t s) {
  if (!R || !r_spatial || !lengths || !rel || !frame_rel || !app_rel) return stlt_set_error(STLT_EINVAL, "stlt_relevance_combine_joint: null pointer");
  if (B < 0 || T < 1 || A < 1 || N < 1 || T > 0x7fffLL || A > 0x7fffLL || N > 0x7fffLL || B > 0x7fffff00LL || B * (T * N + T + A) > 0x7fffff00LL)
    return stlt_set_error(STLT_EINVAL, "stlt_relevance_combine_joint: bad batch shape");
  for (const StltNamedPtr& q : {StltNamedPtr{"R", R}, StltNamedPtr{"r_spatial", r_spatial}, StltNamedPtr{"rel", rel}, StltNamedPtr{"frame_rel", frame_rel},
                                StltNamedPtr{"app_rel", app_rel}})
    if ((uintptr_t)q.p & 3) return stlt_set_error(STLT_EINVAL, "stlt_relevance_combine_joint: %s must be 4-byte aligned", q.name);
  if ((uintptr_t)lengths & 7) return stlt_set_error(STLT_EINVAL, "stlt_relevance_combine_joint: lengths must be 8-byte aligned");
  if (B == 0) return 0;
  CombineGeo g;
  g.R = R; g.r_spatial = r_spatial; g.lengths = lengths; g.rel = rel; g.frame_rel = frame_rel; g.app_rel = app_rel;
  g.B = B; g.T = T; g.A = A; g.N = N; g.w_layout = w_layout; g.w_appearance = w_appearance;
  const int64_t n = B * (T * N + T + A);
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("relevance_combine_joint B=%lld T=%lld A=%lld N=%lld", (long long)B, (long long)T, (long long)A, (long long)N);
  stlt_prof_add_bytes((double)B * T * N * 4.0 * 2 + (double)B * (T + A) * 4.0 * 3);
  hipLaunchKernelGGL(relevance_combine_joint_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g);
  return stlt_check_launch("relevance_combine_joint_kernel");
}

extern "C" {

int stlt_attn_grad_probs(const float* qkv, const float* dctx, const uint8_t* kpm, int causal, int64_t S, int64_t L, int64_t H, int64_t dh, float* abar,
                         stlt_stream_t stream) {
  return launch_attn_grad_probs(qkv, dctx, kpm, causal, S, L, H, dh, abar, (hipStream_t)stream);
}

int stlt_attn_rollout(const float* abar, int64_t n_layers, int64_t S, int64_t L, float* R, stlt_stream_t stream) {
  return launch_attn_rollout(abar, n_layers, S, L, R, (hipStream_t)stream);
}

int stlt_relevance_combine(const float* r_temporal, const float* r_spatial, const int64_t* lengths, int64_t B, int64_t T, int64_t N, float* rel,
                           stlt_stream_t stream) {
  return launch_relevance_combine(r_temporal, r_spatial, lengths, B, T, N, rel, (hipStream_t)stream);
}

int stlt_attn_grad_probs_cross(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* dctx, const uint8_t* kpm, int causal,
                               int64_t S, int64_t Lq, int64_t Lk, int64_t H, int64_t dh, float* abar, stlt_stream_t stream) {
  return launch_attn_grad_probs_cross(q, ldq, k, v, ldkv, dctx, kpm, causal, S, Lq, Lk, H, dh, abar, (hipStream_t)stream);
}

int stlt_attn_rollout_joint(const float* r_layout, const float* r_appearance, const float* layout_to_appearance, const float* appearance_to_layout,
                            const float* fusion_layout, const float* fusion_appearance, int64_t n_fusion, int64_t S, int64_t T, int64_t A, float* R,
                            stlt_stream_t stream) {
  return launch_attn_rollout_joint(r_layout, r_appearance, layout_to_appearance, appearance_to_layout, fusion_layout, fusion_appearance, n_fusion, S, T, A, R,
                                   (hipStream_t)stream);
}

int stlt_relevance_combine_joint(const float* R, const float* r_spatial, const int64_t* lengths, int64_t B, int64_t T, int64_t A, int64_t N, float w_layout,
                                 float w_appearance, float* rel, float* frame_rel, float* app_rel, stlt_stream_t stream) {
  return launch_relevance_combine_joint(R, r_spatial, lengths, B, T, A, N, w_layout, w_appearance, rel, frame_rel, app_rel, (hipStream_t)stream);
}

}  // extern "C"
