// Attention relevance (include/stlt_hip.h: stlt_attn_grad_probs, stlt_attn_rollout, stlt_relevance_combine): the three kernels that turn what
// the input-only reverse sweep already holds in memory — a layer's packed QKV on the tape and dctx, the gradient wrt the attention core's
// output, right before its attention backward — into gradient-weighted attention maps, their rollout through the residual connections and
// the per-object relevance of a prediction (Chefer, Gur, Wolf 2021).  The reference has none of this: on its nn.MultiheadAttention layers
// (models.py:46-55,118-128) it takes need_weights=True, retain_grad on every layer's weights and a Python loop over the layers.
//
//   grad-probs: abar[s,i,j] = (1/H) sum_h max(P_h[s,i,j] * G_h[s,i,j], 0), G_h[s,i,j] = dctx_h[s,i,:] · v_h[s,j,:], P_h what attn_probs.hip
//               computes (same masks, same softmax).  dh == 64 with L <= 64 (every released checkpoint, every layout of the reference): the
//               MFMA kernel described at attn_grad_probs16_kernel below — measured, the vector-ALU kernel alone took 3 to 4 times the attention
//               backward's launch beside it on those shapes (profiles/attention_relevance_bench.md).  Everything else: the generic
//               kernel's structure of attn_probs.hip with a second dot product against V: a group of
//               W lanes (W = the power of two >= L, at most 64) per (sequence, query row), lane = key (keys lane, lane + 64, ...: at most four per
//               lane, in registers), the query row and the dctx row of the group broadcast from LDS, the head loop inside, the heads summed in
//               registers in their order — no atomics, the same bits on every run.  Short sequences (the spatial tower's N = 7) put 64 / W query
//               rows into one wave instead of leaving 57 lanes idle; the rows of a wave lie dh + 4 floats apart in LDS so that the 16-byte reads
//               of different groups fall on different banks.
//   rollout:    R_0 = I, R_l = R_{l-1} + abar_l · R_{l-1}.  The columns of R never mix (column j of R_l depends on column j of R_{l-1} alone), so
//               a workgroup keeps a block of columns of one item's R in LDS, ping-pong, for the WHOLE chain while the layers stream in from
//               memory: one launch whatever the length.  L <= 64: the block is every column, and several items share a workgroup when L is small;
//               64 < L <= 256: blocks of 16 columns, (L, 16) floats a side.  fp32 FMA over k in ascending order.
//   combine:    rel[b,t,n] = R_temporal[b, lengths[b]-1, t] * R_spatial[b,t,0,n]  (row 0 of a frame is its CLS token, models.py:79; the head
//               reads frame lengths-1 of a clip, models.py:189-192).
#include <cmath>
#include <cstdint>
#include "common.h"
#include "attn_vec.h"
#include "wave_dpp.h"

namespace {

constexpr int GP_WAVES = 4;        // independent waves per workgroup
constexpr int GP_MAX_L = 256;      // the attention backward's own domain (backward.hip)
constexpr int GP_MAX_DH = 256;
constexpr int GP_KEYS_PER_LANE = GP_MAX_L / 64;
constexpr int GP_ROW_FLOATS = 512;  // a wave's query rows in LDS: rows * dh <= this ...
constexpr int GP_LDS_FLOATS = GP_ROW_FLOATS + 4 * 64;  // ... plus the four floats of padding behind each of at most 64 rows

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

// ---- MFMA path (dh == 64, L <= 64): attn_probs.hip's attn_probs16_kernel — attn16.hip's dataflow — with its value half back in another role.
// S^T = K·Q^T and G^T = V·dctx^T are the same product on two pairs of operands: v_mfma_f32_16x16x4_f32 with swapped operands, lane (li, lg)
// holding, for query row li of a 16-row block, the scores AND the gradients of keys 4 lg .. 4 lg + 3 of every key block, so p * g meets in
// registers and a row's maximum and sum are in-register plus two exchanges between the four lane groups.  All four fragments come straight
// from global memory in operand shape; no LDS.  FULL (16 < L <= 64): a unit = (sequence, query block) against the NB key blocks (causal: up
// to its own); DIAG (L <= 16): a unit = one 16-row block of P = floor(16 / L) whole sequences, pairs of different sequences masked off.
constexpr int GP16_DH = 64;

struct GradProbs16Geo {
  const float* qkv; const float* dctx; const uint8_t* kpm; float* abar;
  int64_t n_units;
  int n_tokens, L, H, P;  // P = sequences per 16-row block (DIAG), 1 for FULL
  int causal;
  float scale, inv_h;
};

template <int NB, bool FULL>
__global__ __launch_bounds__(64 * GP_WAVES) void attn_grad_probs16_kernel(const GradProbs16Geo geo) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * GP_WAVES + wave;
  if (unit >= geo.n_units) return;  // wave-uniform: no lane of a working wave is ever switched off
  const int H = geo.H, L = geo.L, d = H * GP16_DH;
  const int64_t ld = 3 * (int64_t)d;
  const bool causal = geo.causal != 0;

  const int64_t item = FULL ? unit / NB : unit;
  const int qb = FULL ? (int)(unit - item * NB) : 0;
  const int rows = FULL ? L : geo.P * L;                      // rows of the item
  const int64_t t0 = FULL ? item * L : item * (int64_t)rows;  // its first token
  auto row_token = [&](int local) __attribute__((always_inline)) -> int64_t {
    return (local < rows && t0 + local < geo.n_tokens) ? t0 + local : -1;
  };
  int64_t spare = t0 + rows - 1;  // a valid token to read in place of an absent row (such rows are masked / never stored)
  if (spare > geo.n_tokens - 1) spare = geo.n_tokens - 1;
  auto used = [&](int kb) __attribute__((always_inline)) { return !FULL || !causal || kb <= qb; };

  const int q_local = qb * 16 + li;
  const int64_t q_tok = row_token(q_local);
  const int q_seq = FULL ? 0 : li / L;
  const int q_pos = FULL ? q_local : li - q_seq * L;
  int k_pos[NB][4];
  bool k_col[NB][4];  // the pair (query, key) has a place in the output
  bool k_ok[NB][4];   // ... and is not masked
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k_local = kb * 16 + 4 * lg + r;
      const int64_t k_tok = row_token(k_local);
      const int k_seq = FULL ? 0 : k_local / L;
      k_pos[kb][r] = FULL ? k_local : k_local - k_seq * L;
      k_col[kb][r] = q_tok >= 0 && k_tok >= 0 && k_seq == q_seq;
      const bool padded = geo.kpm[k_tok >= 0 ? k_tok : spare] != 0;
      k_ok[kb][r] = k_col[kb][r] && !padded && (!causal || k_pos[kb][r] <= q_pos);
    }
  }

  f32x4 kf[NB][4], vf[NB][4], qc[4], gc[4];
  auto load_head = [&](int head) __attribute__((always_inline)) {
    const int col = head * GP16_DH + 4 * lg;
    const int64_t qt = q_tok >= 0 ? q_tok : spare;
    const float* qrow = geo.qkv + qt * ld + col;
    const float* grow = geo.dctx + qt * d + col;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      qc[c] = *reinterpret_cast<const f32x4*>(qrow + 16 * c);
      gc[c] = *reinterpret_cast<const f32x4*>(grow + 16 * c);
    }
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      if (!used(kb)) continue;
      const int64_t tok = row_token(kb * 16 + li);
      const float* krow = geo.qkv + (tok >= 0 ? tok : spare) * ld + d + col;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        kf[kb][c] = *reinterpret_cast<const f32x4*>(krow + 16 * c);
        vf[kb][c] = *reinterpret_cast<const f32x4*>(krow + d + 16 * c);
      }
    }
  };

  f32x4 acc[NB];
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
  load_head(0);
  for (int head = 0; head < H; ++head) {
    // ---- st[kb][r] = score, gt[kb][r] = gradient of key kb*16 + 4*lg + r against query qb*16 + li
    f32x4 st[NB], gt[NB];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      st[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
      gt[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (used(kb)) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            st[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][c][e], qc[c][e], st[kb], 0, 0, 0);
            gt[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[kb][c][e], gc[c][e], gt[kb], 0, 0, 0);
          }
      }
    }
    if (head + 1 < H) load_head(head + 1);  // the fragment registers are dead: the next head's loads go under the softmax
    float m = -1e30f;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[kb][r] = k_ok[kb][r] ? st[kb][r] * geo.scale : -1e30f;
        m = fmaxf(m, st[kb][r]);
      }
    m = groups_max(m);
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = st[kb][r] > -1e29f ? __expf(st[kb][r] - m) : 0.f;
        st[kb][r] = p;
        sum += p;
      }
    sum = groups_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;  // fully masked row -> zeros
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[kb][r] += k_ok[kb][r] ? fmaxf(st[kb][r] * inv * gt[kb][r], 0.f) : 0.f;
  }
  // row q_pos of the query's sequence's (L, L) map; four-byte stores (a row of L floats is not 16-byte aligned for L = 7)
  const int64_t seq = FULL ? item : item * geo.P + q_seq;
  float* const out_row = geo.abar + seq * L * L + (int64_t)q_pos * L;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (k_col[kb][r]) out_row[k_pos[kb][r]] = acc[kb][r] * geo.inv_h;
}

template <int NB, bool FULL>
void launch_grad_probs16(const GradProbs16Geo& g, unsigned n_wg, hipStream_t s) {
  hipLaunchKernelGGL((attn_grad_probs16_kernel<NB, FULL>), dim3(n_wg), dim3(64 * GP_WAVES), 0, s, g);
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
      float a = old[e];
      if (item < geo.S) {  // (the items past the end keep their identity and are never stored)
        const float* arow = geo.abar + ((int64_t)l * geo.S + item) * map + (int64_t)i * L;
        const float* col = old + p * tile + j;
        for (int k = 0; k < L; ++k) a = fmaf(arow[k], col[k * CB], a);
      }
      nxt[e] = a;
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
  const bool mfma = dh == GP16_DH && L <= 64;
  if (mfma) {
    GradProbs16Geo m;
    m.qkv = qkv; m.dctx = dctx; m.kpm = kpm; m.abar = abar;
    m.n_tokens = (int)(S * L); m.L = (int)L; m.H = (int)H; m.P = L <= 16 ? (int)(16 / L) : 1;
    m.causal = g.causal; m.scale = g.scale; m.inv_h = g.inv_h;
    const int nb = (int)((L + 15) / 16);
    m.n_units = L <= 16 ? (S + m.P - 1) / m.P : S * nb;
    const int64_t wgs = (m.n_units + GP_WAVES - 1) / GP_WAVES;  // <= S * 4: below 2^31
    StltProfScope ps(STLT_K_ATTN_PROBS, s);
    stlt_prof_note("attn_grad_probs %s S=%lld L=%lld H=%lld dh=%lld causal=%d", L <= 16 ? "mfma-diag" : "mfma-full", (long long)S, (long long)L, (long long)H,
                   (long long)dh, g.causal);
    stlt_prof_add_bytes((double)S * L * H * dh * 4.0 * 4 + (double)S * L * L * 4.0 + (double)S * L);  // q, k, v, dctx, abar, mask
    stlt_prof_note_flops((double)S * H * L * L * 4.0 * dh * (causal ? 0.5 : 1.0));
    if (L <= 16) launch_grad_probs16<1, false>(m, (unsigned)wgs, s);
    else if (nb == 2) launch_grad_probs16<2, true>(m, (unsigned)wgs, s);
    else if (nb == 3) launch_grad_probs16<3, true>(m, (unsigned)wgs, s);
    else launch_grad_probs16<4, true>(m, (unsigned)wgs, s);
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

int launch_attn_rollout(const float* abar, int64_t n_layers, int64_t S, int64_t L, float* R, hipStream_t s) {
  if (!R || (n_layers > 0 && !abar)) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: null pointer");
  if (n_layers < 0 || n_layers > 64) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: layer count %lld unsupported (0 ... 64)", (long long)n_layers);
  if (L < 1 || L > GP_MAX_L) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout: sequence length %lld unsupported (1 ... %d)", (long long)L, GP_MAX_L);
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

}  // extern "C"
