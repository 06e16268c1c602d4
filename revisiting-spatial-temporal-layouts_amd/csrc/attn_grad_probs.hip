// Gradient-weighted attention maps (include/stlt_hip.h: stlt_attn_grad_probs, stlt_attn_grad_probs_cross): the kernels that turn what the
// input-only reverse sweep already holds in memory — a layer's projected Q / K / V on the tape and dctx, the gradient wrt the attention core's
// output, right before its attention backward — into the maps attn_rollout.hip rolls out (Chefer, Gur, Wolf 2021).  The reference has none
// of this: on its nn.MultiheadAttention layers (models.py:46-55,118-128, and the CrossAttentionLayer of models.py:362-382) it takes
// need_weights=True, retain_grad on every layer's weights and a Python loop over the layers.
//
//   abar[s,i,j] = (1/H) sum_h max(P_h[s,i,j] * G_h[s,i,j], 0), G_h[s,i,j] = dctx_h[s,i,:] · v_h[s,j,:], P_h what attn_probs.hip computes (same
//   masks, same softmax).  Two launchers: a packed QKV buffer (one tower), and queries and keys / values in different buffers and of
//   different number (the fusion models' blocks, CrossAttentionLayer called at models.py:411-419).
//
//   MFMA    (dh == 64, at most 64 keys — every released checkpoint, every layout and fusion block of the reference): attn_grad_probs16_kernel
//           below, on either geometry of attn_rows16.h — measured, the vector-ALU kernel alone took 3 to 4 times the attention backward's
//           launch beside it on those shapes (profiles/attention_relevance_bench.md).  The cross launcher sends a launch of fewer than 128
//           units over three or four key blocks to its vector kernel, which measured faster there (launcher).
//   generic, packed: the generic kernel's structure of attn_probs.hip with a second dot product against V: a group of
//           W lanes (W = the power of two >= L, at most 64) per (sequence, query row), lane = key (keys lane, lane + 64, ...: at most four per
//           lane, in registers), the query row and the dctx row of the group broadcast from LDS, the head loop inside, the heads summed in
//           registers in their order — no atomics, the same bits on every run.  Short sequences (the spatial tower's N = 7) put 64 / W query
//           rows into one wave instead of leaving 57 lanes idle; the rows of a wave lie dh + 4 floats apart in LDS so that the 16-byte reads
//           of different groups fall on different banks.
//   generic, cross: one wave per (sequence, query row), lane = key (keys lane, lane + 64, ...), the query row and the dctx row broadcast
//           from LDS.  Heads summed in their order in registers, no atomics.  (The two generic kernels reduce in different orders and have
//           different occupancies: they are not one kernel on two views.)
#include <cmath>
#include <cstdint>
#include "common.h"
#include "attn_vec.h"
#include "attn_rows16.h"

namespace {

constexpr int GP_DH = 64;          // head dim of the MFMA path
constexpr int GP_WAVES = 4;        // independent waves per workgroup
constexpr int GP_MAX_L = 256;      // the attention backward's own domain (backward.hip)
constexpr int GP_MAX_DH = 256;
constexpr int GP_KEYS_PER_LANE = GP_MAX_L / 64;
constexpr int GP_ROW_FLOATS = 512;  // a wave's query rows in LDS: rows * dh <= this ...
constexpr int GP_LDS_FLOATS = GP_ROW_FLOATS + 4 * 64;  // ... plus the four floats of padding behind each of at most 64 rows
constexpr int GX_MIN_UNITS = 128;  // below this many units a cross launch over three or four key blocks goes to the vector kernel (launcher)

struct GradProbsGeo {
  const float* qkv;    // packed (S*L, 3*H*dh): q | k | v
  const float* dctx;   // (S*L, H*dh)
  const uint8_t* kpm;  // one byte per token: 1 = padded key
  float* abar;         // (S, L, L)
  int64_t n_rows;      // S * L query rows
  int L, H, dh, W, G;  // W lanes per query row, G query rows per wave
  int causal;
  float scale, inv_h;
};

struct GradCrossGeo {
  const float* q;      // (S*Lq, ldq), the first H*dh columns
  const float* k;      // (S*Lk, ldkv), the first H*dh columns
  const float* v;      // (S*Lk, ldkv), the first H*dh columns
  const float* dctx;   // (S*Lq, H*dh)
  const uint8_t* kpm;  // (S*Lk): 1 = padded key
  float* abar;         // (S, Lq, Lk)
  int64_t ldq, ldkv, n_units;
  int Lq, Lk, H, dh, nqb;  // nqb = query blocks per sequence (MFMA)
  int causal;
  float scale, inv_h;
  int P, n_tokens;     // MFMA on a packed buffer with L <= 16: sequences per 16-row block, S * L (read by DiagRows alone: the sided and vector kernels ignore both)
};

// max / sum over the W lanes of a group (W a power of two: lanes ^ o with o < W stay inside the group); every step pairs the same two
// numbers on every run
__device__ __forceinline__ float group_max(float x, int W) {
  for (int o = W >> 1; o >= 1; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  return x;
}
__device__ __forceinline__ float group_sum(float x, int W) {
  for (int o = W >> 1; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// ---- MFMA path: attn_probs.hip's attn_probs16_kernel with its value half back in another role.  S^T = K·Q^T and G^T = V·dctx^T are the same
// product on two pairs of operands: lane (li, lg) holds, for query row li of a 16-row block, the scores AND the gradients of keys
// 4 lg .. 4 lg + 3 of every key block, so p * g meets in registers.  All four fragments come straight from global memory in operand shape.
template <int NB, class Rows>
__global__ __launch_bounds__(64 * GP_WAVES) void attn_grad_probs16_kernel(const GradCrossGeo geo) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * GP_WAVES + wave;
  if (unit >= geo.n_units) return;  // wave-uniform: no lane of a working wave is ever switched off
  const int H = geo.H;
  const int64_t d = (int64_t)H * GP_DH;
  const bool causal = geo.causal != 0;
  const Rows rows(geo, unit);
  const int q_local = rows.qb * 16 + li;
  const Keys16<NB> keys(rows, q_local, lg, geo.kpm, causal);

  f32x4 kf[NB][4], vf[NB][4], qc[4], gc[4];
  auto load_head = [&](int head) __attribute__((always_inline)) {
    const int col = head * GP_DH + 4 * lg;
    const int64_t qt = q_read(rows, q_local);
    load_frag16(qc, geo.q + qt * geo.ldq + col);
    load_frag16(gc, geo.dctx + qt * d + col);
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      if (!rows.used(kb, causal)) continue;
      const int64_t off = k_read(rows, kb * 16 + li) * geo.ldkv + col;
      load_frag16(kf[kb], geo.k + off);
      load_frag16(vf[kb], geo.v + off);
    }
  };

  f32x4 acc[NB];
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
  load_head(0);
  for (int head = 0; head < H; ++head) {
    f32x4 st[NB], gt[NB];  // st[kb][r] = score, gt[kb][r] = gradient of key kb*16 + 4*lg + r against query q_local
    scores16<NB>(rows, causal, kf, qc, st);
    scores16<NB>(rows, causal, vf, gc, gt);
    if (head + 1 < H) load_head(head + 1);  // the fragment registers are dead: the next head's loads go under the softmax
    const float inv = softmax16<NB>(st, keys.ok, geo.scale);
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[kb][r] += keys.ok[kb][r] ? fmaxf(st[kb][r] * inv * gt[kb][r], 0.f) : 0.f;
  }
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) acc[kb] = acc[kb] * geo.inv_h;
  // the query's row of its sequence's (Lq, Lk) map
  store_row16<NB>(geo.abar + rows.out_seq(keys.q_seq) * geo.Lq * geo.Lk + (int64_t)keys.q_pos * geo.Lk, acc, keys);
}

// the MFMA kernel over the two-sided geometry for nb key blocks
void launch_grad_probs_sided(const GradCrossGeo& g, int nb, unsigned n_wg, hipStream_t s) {
  const dim3 block(64 * GP_WAVES);
  if (nb == 1) hipLaunchKernelGGL((attn_grad_probs16_kernel<1, SidedRows>), dim3(n_wg), block, 0, s, g);
  else if (nb == 2) hipLaunchKernelGGL((attn_grad_probs16_kernel<2, SidedRows>), dim3(n_wg), block, 0, s, g);
  else if (nb == 3) hipLaunchKernelGGL((attn_grad_probs16_kernel<3, SidedRows>), dim3(n_wg), block, 0, s, g);
  else hipLaunchKernelGGL((attn_grad_probs16_kernel<4, SidedRows>), dim3(n_wg), block, 0, s, g);
}

// ---- generic path.  KPL keys per lane: 1 while L <= 64 (then W may be below 64), GP_KEYS_PER_LANE above (W == 64, G == 1)
template <bool VEC, int KPL>
__global__ __launch_bounds__(64 * GP_WAVES) void attn_grad_probs_kernel(const GradProbsGeo geo) {
  __shared__ __attribute__((aligned(16))) float q_lds[GP_WAVES][GP_LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float g_lds[GP_WAVES][GP_LDS_FLOATS];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int L = geo.L, H = geo.H, dh = geo.dh, W = geo.W, G = geo.G;
  const int64_t row0 = ((int64_t)blockIdx.x * GP_WAVES + wave) * G;  // first query token of the wave
  if (row0 >= geo.n_rows) return;                                    // wave-uniform
  float* qs = q_lds[wave];
  float* gs = g_lds[wave];
  const int64_t d = (int64_t)H * dh, ld = 3 * d;
  const int stride = dh + 4;  // LDS row pitch
  const int sub = lane / W, kl = lane - sub * W;
  const int64_t row = row0 + sub;
  const bool live = sub < G && row < geo.n_rows;  // this lane's group has a query row (the others only take part in the exchanges)
  const int64_t seq = live ? row / L : 0;
  const int i = live ? (int)(row - seq * L) : 0;
  const int64_t k_base = seq * L;
  bool ok[KPL];
  float acc[KPL];
#pragma unroll
  for (int t = 0; t < KPL; ++t) {
    const int j = kl + 64 * t;
    ok[t] = live && j < L && geo.kpm[k_base + (j < L ? j : 0)] == 0 && (!geo.causal || j <= i);
    acc[t] = 0.f;
  }
  const int n_rows_here = (int)(geo.n_rows - row0 < G ? geo.n_rows - row0 : G);
  for (int head = 0; head < H; ++head) {
    wave_lds_sync();  // the previous head's reads of qs / gs are done
    for (int e = lane; e < n_rows_here * dh; e += 64) {
      const int r = e / dh, c = e - r * dh;
      qs[r * stride + c] = geo.qkv[(row0 + r) * ld + (int64_t)head * dh + c];
      gs[r * stride + c] = geo.dctx[(row0 + r) * d + (int64_t)head * dh + c];
    }
    wave_lds_sync();
    float sc[KPL], gr[KPL];
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < KPL; ++t) {
      sc[t] = -1e30f;
      gr[t] = 0.f;
      if (64 * t < L) {  // wave-uniform
        if (ok[t]) {
          const float* krow = geo.qkv + (k_base + kl + 64 * t) * ld + d + (int64_t)head * dh;
          sc[t] = dot_row<VEC>(qs + sub * stride, krow, dh) * geo.scale;
          gr[t] = dot_row<VEC>(gs + sub * stride, krow + d, dh);  // the value row of the same key
        }
        mx = fmaxf(mx, sc[t]);
      }
    }
    mx = group_max(mx, W);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < KPL; ++t) {
      sc[t] = sc[t] > -1e29f ? expf(sc[t] - mx) : 0.f;
      sum += sc[t];
    }
    sum = group_sum(sum, W);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;  // fully masked row -> zeros
#pragma unroll
    for (int t = 0; t < KPL; ++t) acc[t] += ok[t] ? fmaxf(sc[t] * inv * gr[t], 0.f) : 0.f;
  }
  if (live) {
    float* const out_row = geo.abar + row * L;  // (S, L, L): row (seq, i)
#pragma unroll
    for (int t = 0; t < KPL; ++t)
      if (kl + 64 * t < L) out_row[kl + 64 * t] = acc[t] * geo.inv_h;
  }
}

// one wave per (sequence, query row): keys lane, lane + 64, ... in registers, the head loop inside
template <bool VEC>
__global__ __launch_bounds__(64 * GP_WAVES) void attn_grad_probs_cross_any_kernel(const GradCrossGeo geo) {
  __shared__ __attribute__((aligned(16))) float q_lds[GP_WAVES][GP_MAX_DH];
  __shared__ __attribute__((aligned(16))) float g_lds[GP_WAVES][GP_MAX_DH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * GP_WAVES + wave;  // query token
  if (row >= geo.n_units) return;
  float* qs = q_lds[wave];
  float* gs = g_lds[wave];
  const int Lq = geo.Lq, Lk = geo.Lk, H = geo.H, dh = geo.dh;
  const int64_t d = (int64_t)H * dh;
  const int64_t seq = row / Lq;
  const int i = (int)(row - seq * Lq);
  const int64_t k_base = seq * Lk;
  bool ok[GP_KEYS_PER_LANE];
  float acc[GP_KEYS_PER_LANE];
#pragma unroll
  for (int t = 0; t < GP_KEYS_PER_LANE; ++t) {
    const int j = lane + 64 * t;
    ok[t] = j < Lk && geo.kpm[k_base + (j < Lk ? j : 0)] == 0 && (!geo.causal || j <= i);
    acc[t] = 0.f;
  }
  for (int head = 0; head < H; ++head) {
    const float* qrow = geo.q + row * geo.ldq + (int64_t)head * dh;
    const float* grow = geo.dctx + row * d + (int64_t)head * dh;
    wave_lds_sync();  // the previous head's reads of qs / gs are done
    for (int c = lane; c < dh; c += 64) {
      qs[c] = qrow[c];
      gs[c] = grow[c];
    }
    wave_lds_sync();
    float sc[GP_KEYS_PER_LANE], gr[GP_KEYS_PER_LANE];
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < GP_KEYS_PER_LANE; ++t) {
      sc[t] = -1e30f;
      gr[t] = 0.f;
      if (64 * t < Lk) {  // wave-uniform
        if (ok[t]) {
          const int64_t off = (k_base + lane + 64 * t) * geo.ldkv + (int64_t)head * dh;
          sc[t] = dot_row<VEC>(qs, geo.k + off, dh) * geo.scale;
          gr[t] = dot_row<VEC>(gs, geo.v + off, dh);  // the value row of the same key
        }
        mx = fmaxf(mx, sc[t]);
      }
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < GP_KEYS_PER_LANE; ++t) {
      sc[t] = sc[t] > -1e29f ? expf(sc[t] - mx) : 0.f;
      sum += sc[t];
    }
    sum = wave_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;  // fully masked row -> zeros
#pragma unroll
    for (int t = 0; t < GP_KEYS_PER_LANE; ++t) acc[t] += ok[t] ? fmaxf(sc[t] * inv * gr[t], 0.f) : 0.f;
  }
  float* const out_row = geo.abar + row * Lk;  // (S, Lq, Lk): row (seq, i)
#pragma unroll
  for (int t = 0; t < GP_KEYS_PER_LANE; ++t)
    if (lane + 64 * t < Lk) out_row[lane + 64 * t] = acc[t] * geo.inv_h;
}

}  // namespace

int launch_attn_grad_probs(const float* qkv, const float* dctx, const uint8_t* kpm, int causal, int64_t S, int64_t L, int64_t H, int64_t dh, float* abar,
                           hipStream_t s) {
  if (!qkv || !dctx || !kpm || !abar) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: null pointer");
  if (L < 1 || L > GP_MAX_L) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: sequence length %lld unsupported (1 ... %d)", (long long)L, GP_MAX_L);
  if (dh < 1 || dh > GP_MAX_DH) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: head dim %lld unsupported (1 ... %d)", (long long)dh, GP_MAX_DH);
  if (S < 0 || S > 0x7fffff00LL || H <= 0 || H > 65535 || S * L > 0x7fffff00LL) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: bad sequence / head count");
  const bool vec = dh % 4 == 0;  // every q / k / v / dctx slice of a row then starts on 16 bytes when the buffers do
  if (vec) {
    if (const char* off = stlt_first_unaligned16({{"qkv", qkv}, {"dctx", dctx}})) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: %s must be 16-byte aligned", off);
  }
  if ((uintptr_t)qkv & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: qkv must be 4-byte aligned");
  if ((uintptr_t)dctx & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: dctx must be 4-byte aligned");
  if ((uintptr_t)abar & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: abar must be 4-byte aligned");
  if (S == 0) return 0;
  GradProbsGeo g;
  g.qkv = qkv; g.dctx = dctx; g.kpm = kpm; g.abar = abar;
  g.n_rows = S * L; g.L = (int)L; g.H = (int)H; g.dh = (int)dh;
  g.causal = causal ? 1 : 0;
  g.scale = 1.0f / sqrtf((float)dh);
  g.inv_h = 1.0f / (float)H;
  const bool mfma = dh == GP_DH && L <= 64;
  if (mfma) {
    const int64_t d = H * dh;
    const int nb = (int)((L + 15) / 16);
    GradCrossGeo m;  // the packed buffer as two sides
    m.q = qkv; m.k = qkv + d; m.v = qkv + 2 * d; m.dctx = dctx; m.kpm = kpm; m.abar = abar; m.ldq = m.ldkv = 3 * d;
    m.Lq = m.Lk = (int)L; m.H = (int)H; m.dh = (int)dh; m.nqb = nb;
    m.n_tokens = (int)(S * L); m.P = L <= 16 ? (int)(16 / L) : 1;
    m.causal = g.causal; m.scale = g.scale; m.inv_h = g.inv_h;
    m.n_units = L <= 16 ? (S + m.P - 1) / m.P : S * nb;
    const int64_t wgs = (m.n_units + GP_WAVES - 1) / GP_WAVES;  // <= S * 4: below 2^31
    StltProfScope ps(STLT_K_ATTN_PROBS, s);
    stlt_prof_note("attn_grad_probs %s S=%lld L=%lld H=%lld dh=%lld causal=%d", L <= 16 ? "mfma-diag" : "mfma-full", (long long)S, (long long)L, (long long)H,
                   (long long)dh, g.causal);
    stlt_prof_add_bytes((double)S * L * H * dh * 4.0 * 4 + (double)S * L * L * 4.0 + (double)S * L);  // q, k, v, dctx, abar, mask
    stlt_prof_note_flops((double)S * H * L * L * 4.0 * dh * (causal ? 0.5 : 1.0));
    if (L <= 16) hipLaunchKernelGGL((attn_grad_probs16_kernel<1, DiagRows>), dim3((unsigned)wgs), dim3(64 * GP_WAVES), 0, s, m);
    else launch_grad_probs_sided(m, nb, (unsigned)wgs, s);
    return stlt_check_launch("attn_grad_probs16_kernel");
  }
  int W = 1;
  while (W < L && W < 64) W *= 2;
  g.W = W;
  g.G = 64 / W < GP_ROW_FLOATS / (int)dh ? 64 / W : GP_ROW_FLOATS / (int)dh;  // >= 1: dh <= 256
  const int64_t n_waves = (g.n_rows + g.G - 1) / g.G;
  const int64_t n_wg = (n_waves + GP_WAVES - 1) / GP_WAVES;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs: too many work items");
  StltProfScope ps(STLT_K_ATTN_PROBS, s);
  stlt_prof_note("attn_grad_probs generic S=%lld L=%lld H=%lld dh=%lld causal=%d rows/wave=%d", (long long)S, (long long)L, (long long)H, (long long)dh, g.causal, g.G);
  stlt_prof_add_bytes((double)S * L * H * dh * 4.0 * 4 + (double)S * L * L * 4.0 + (double)S * L);  // q, k, v, dctx, abar, mask
  stlt_prof_note_flops((double)S * H * L * L * 4.0 * dh * (causal ? 0.5 : 1.0));
  const dim3 grid((unsigned)n_wg), block(64 * GP_WAVES);
  if (L <= 64) {
    if (vec) hipLaunchKernelGGL((attn_grad_probs_kernel<true, 1>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((attn_grad_probs_kernel<false, 1>), grid, block, 0, s, g);
  } else {
    if (vec) hipLaunchKernelGGL((attn_grad_probs_kernel<true, GP_KEYS_PER_LANE>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((attn_grad_probs_kernel<false, GP_KEYS_PER_LANE>), grid, block, 0, s, g);
  }
  return stlt_check_launch("attn_grad_probs_kernel");
}

int launch_attn_grad_probs_cross(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* dctx, const uint8_t* kpm, int causal,
                                 int64_t S, int64_t Lq, int64_t Lk, int64_t H, int64_t dh, float* abar, hipStream_t s) {
  if (!q || !k || !v || !dctx || !kpm || !abar) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: null pointer");
  if (Lq < 1 || Lq > GP_MAX_L || Lk < 1 || Lk > GP_MAX_L)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: sequence lengths %lld / %lld unsupported (1 ... %d)", (long long)Lq, (long long)Lk, GP_MAX_L);
  if (dh < 1 || dh > GP_MAX_DH) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: head dim %lld unsupported (1 ... %d)", (long long)dh, GP_MAX_DH);
  if (S < 0 || S > 0x7fffff00LL || H <= 0 || H > 65535 || S * Lq > 0x7fffff00LL || S * Lk > 0x7fffff00LL)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: bad sequence / head count");
  if (causal && Lq != Lk) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: causal needs Lq == Lk (%lld, %lld)", (long long)Lq, (long long)Lk);
  if (ldq < H * dh || ldkv < H * dh || ldq > 0x7fffffffLL || ldkv > 0x7fffffffLL)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: ldq / ldkv must be at least H * dh");
  const bool mfma_shape = dh == GP_DH && Lk <= 64;
  const int64_t nqb = (Lq + 15) / 16, nb = (Lk + 15) / 16;
  // Measured (profiles/fusion_relevance_bench.md §3): an MFMA unit is ONE wave that walks its key blocks and all heads alone, so a launch of few
  // units with three or four key blocks leaves the chip empty and the vector kernel's S * Lq waves finish first — 64 units x 3 blocks (16
  // frames against 33 appearance tokens at 64 clips): 43 us against 39 us; from 128 units on, and at one or two key blocks, the MFMA kernel wins.
  const bool few_units = S * nqb < GX_MIN_UNITS && nb >= 3;
#ifdef STLT_GRAD_PROBS_CROSS_NO_MFMA  // the A/B build of tools/bench_fusion_relevance.py (build.variant): every shape on the vector-ALU kernel,
  const bool mfma = false;            // the header's contract (alignment refusals included) unchanged
#elif defined(STLT_GRAD_PROBS_CROSS_ALL_MFMA)  // ... and every MFMA shape on the MFMA kernel, however few its units
  const bool mfma = mfma_shape;
#else
  const bool mfma = mfma_shape && !few_units;
#endif
  const uintptr_t ptrs = (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dctx;
  if (mfma_shape && ((ptrs & 15) || (ldq & 3) || (ldkv & 3)))
    return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: q, k, v and dctx must be 16-byte aligned and ldq, ldkv multiples of 4 at head dim 64 with Lk <= 64");
  if (ptrs & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: q, k, v and dctx must be 4-byte aligned");
  if ((uintptr_t)abar & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: abar must be 4-byte aligned");
  if (S == 0) return 0;
  GradCrossGeo g;
  g.q = q; g.k = k; g.v = v; g.dctx = dctx; g.kpm = kpm; g.abar = abar; g.ldq = ldq; g.ldkv = ldkv;
  g.Lq = (int)Lq; g.Lk = (int)Lk; g.H = (int)H; g.dh = (int)dh;
  g.causal = causal ? 1 : 0;
  g.scale = 1.0f / sqrtf((float)dh);
  g.inv_h = 1.0f / (float)H;
  g.nqb = (int)nqb; g.P = 1; g.n_tokens = (int)(S * Lk);
  g.n_units = mfma ? S * g.nqb : S * Lq;
  const int64_t n_wg = (g.n_units + GP_WAVES - 1) / GP_WAVES;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: too many work items");
  StltProfScope ps(STLT_K_ATTN_PROBS, s);
  stlt_prof_note("attn_grad_probs_cross %s S=%lld Lq=%lld Lk=%lld H=%lld dh=%lld causal=%d", mfma ? "mfma-full" : "generic", (long long)S, (long long)Lq, (long long)Lk,
                 (long long)H, (long long)dh, g.causal);
  stlt_prof_add_bytes((double)S * (Lq + Lk) * H * dh * 4.0 * 2 + (double)S * Lq * Lk * 4.0 + (double)S * Lk);  // q, dctx, k, v, abar, mask
  stlt_prof_note_flops((double)S * H * Lq * Lk * 4.0 * dh * (causal ? 0.5 : 1.0));
  if (mfma) {
    launch_grad_probs_sided(g, (int)nb, (unsigned)n_wg, s);
    return stlt_check_launch("attn_grad_probs16_kernel");
  }
  const bool vec = dh % 4 == 0 && (ptrs & 15) == 0 && (ldq & 3) == 0 && (ldkv & 3) == 0;  // every q / k / v / dctx slice then starts on 16 bytes
  if (vec) hipLaunchKernelGGL((attn_grad_probs_cross_any_kernel<true>), dim3((unsigned)n_wg), dim3(64 * GP_WAVES), 0, s, g);
  else hipLaunchKernelGGL((attn_grad_probs_cross_any_kernel<false>), dim3((unsigned)n_wg), dim3(64 * GP_WAVES), 0, s, g);
  return stlt_check_launch("attn_grad_probs_cross_any_kernel");
}
