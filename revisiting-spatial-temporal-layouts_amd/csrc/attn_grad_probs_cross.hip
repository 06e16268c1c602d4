// Attention relevance across two token sets (include/stlt_hip.h: stlt_attn_grad_probs_cross, stlt_attn_rollout_joint,
// stlt_relevance_combine_joint): what attn_grad_probs.hip does for one tower, for the fusion models' blocks, whose queries and keys lie in
// different buffers and differ in number (CrossAttentionLayer, reference models.py:362-382, called at 411-419), and whose residual stream
// runs over two modalities that attend to each other (CrossModalModule, models.py:403-431).  The reference has none of this.
//
//   grad-probs: abar[s,i,j] = (1/H) sum_h max(P_h[s,i,j] * G_h[s,i,j], 0), G_h[s,i,j] = dctx_h[s,i,:] · v_h[s,j,:], P_h what attn_probs_cross.hip
//               computes.  dh == 64 with Lk <= 64 (any Lq — every fusion block of the reference's shapes, T <= 64 and A = 33): the dataflow of
//               attn_grad_probs.hip's attn_grad_probs16_kernel (S^T = K·Q^T and G^T = V·dctx^T on v_mfma_f32_16x16x4_f32, p * g meeting in
//               registers) with the operand addressing of attn_probs_cross16_kernel (a row -> token map and a spare token per side, Lq only
//               sets the number of units, the output row stride is Lk) — except a launch of fewer than 128 units over three or four key
//               blocks, where the vector kernel measured faster (launcher).  Everything else: one wave per (sequence, query row) on the vector
//               ALU, lane = key (keys lane, lane + 64, ...), the query row and the dctx row broadcast from LDS.  Heads summed in their order in
//               registers, no atomics.
//   rollout:    R over the J = T + A stacked tokens, R_0 = blockdiag(r_layout, r_appearance), then per fusion layer three steps R <- R + X·R with
//               X = [[0, l2a], [a2l, 0]], blockdiag(f_layout, f_appearance[.,0]), blockdiag(0, f_appearance[.,1]).  Only the non-zero quadrants are
//               read.  The columns of R never mix, so a workgroup keeps 16 columns of one item's R in LDS, ping-pong, for the whole chain: one
//               launch; 2 x 512 x 16 floats = 64 KB at the largest J.  fp32 FMA over k in ascending order.
//   combine:    row[b,:] = w_layout R[b, lengths[b]-1, :] + w_appearance R[b, T, :] (the frame the layout head reads, models.py:189-192, and the
//               appearance CLS token, models.py:260-262); frame_rel = row[:T], app_rel = row[T:], rel[b,t,n] = frame_rel[b,t] * r_spatial[b,t,0,n].
#include <cmath>
#include <cstdint>
#include "common.h"
#include "attn_vec.h"
#include "wave_dpp.h"

namespace {

constexpr int GX_DH = 64;     // head dim of the MFMA path
constexpr int GX_WAVES = 4;   // independent waves per workgroup (both paths)
constexpr int GX_MAX_L = 256;  // the attention backward's own domain (backward.hip)
constexpr int GX_MAX_DH = 256;
constexpr int GX_KEYS_PER_LANE = GX_MAX_L / 64;
constexpr int GX_MIN_UNITS = 128;  // below this many units a launch over three or four key blocks goes to the vector kernel (launcher)

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
};

// lane (li, lg) holds, for query row li of a 16-row block, the scores AND the gradients of keys 4 lg .. 4 lg + 3 of every key block
template <int NB>
__global__ __launch_bounds__(64 * GX_WAVES) void attn_grad_probs_cross16_kernel(const GradCrossGeo geo) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * GX_WAVES + wave;
  if (unit >= geo.n_units) return;  // wave-uniform: no lane of a working wave is ever switched off
  const int H = geo.H, Lq = geo.Lq, Lk = geo.Lk;
  const int64_t d = (int64_t)H * GX_DH;
  const bool causal = geo.causal != 0;

  const int64_t seq = unit / geo.nqb;
  const int qb = (int)(unit - seq * geo.nqb);
  const int64_t q0 = seq * Lq, k0 = seq * Lk;  // the sequence's first query / key token
  // local row -> token of each side, -1 = no such row; absent rows read the side's spare token (they are masked / never stored)
  auto q_token = [&](int local) __attribute__((always_inline)) -> int64_t { return local < Lq ? q0 + local : -1; };
  auto k_token = [&](int local) __attribute__((always_inline)) -> int64_t { return local < Lk ? k0 + local : -1; };
  const int64_t q_spare = q0 + Lq - 1, k_spare = k0 + Lk - 1;
  auto used = [&](int kb) __attribute__((always_inline)) { return !causal || kb <= qb; };  // causal: Lq == Lk

  const int q_pos = qb * 16 + li;
  const int64_t q_tok = q_token(q_pos);
  int k_pos[NB][4];
  bool k_col[NB][4];  // the pair (query, key) has a place in the output
  bool k_ok[NB][4];   // ... and is not masked
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      k_pos[kb][r] = kb * 16 + 4 * lg + r;
      const int64_t k_tok = k_token(k_pos[kb][r]);
      k_col[kb][r] = q_tok >= 0 && k_tok >= 0;
      const bool padded = geo.kpm[k_tok >= 0 ? k_tok : k_spare] != 0;
      k_ok[kb][r] = k_col[kb][r] && !padded && (!causal || k_pos[kb][r] <= q_pos);
    }
  }

  f32x4 kf[NB][4], vf[NB][4], qc[4], gc[4];
  auto load_head = [&](int head) __attribute__((always_inline)) {
    const int col = head * GX_DH + 4 * lg;
    const int64_t qt = q_tok >= 0 ? q_tok : q_spare;
    const float* qrow = geo.q + qt * geo.ldq + col;
    const float* grow = geo.dctx + qt * d + col;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      qc[c] = *reinterpret_cast<const f32x4*>(qrow + 16 * c);
      gc[c] = *reinterpret_cast<const f32x4*>(grow + 16 * c);
    }
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      if (!used(kb)) continue;
      const int64_t tok = k_token(kb * 16 + li);
      const int64_t off = (tok >= 0 ? tok : k_spare) * geo.ldkv + col;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        kf[kb][c] = *reinterpret_cast<const f32x4*>(geo.k + off + 16 * c);
        vf[kb][c] = *reinterpret_cast<const f32x4*>(geo.v + off + 16 * c);
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
  // row q_pos of the sequence's (Lq, Lk) map; four-byte stores (a row of Lk floats is not 16-byte aligned for Lk = 33)
  float* const out_row = geo.abar + seq * Lq * Lk + (int64_t)q_pos * Lk;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (k_col[kb][r]) out_row[k_pos[kb][r]] = acc[kb][r] * geo.inv_h;
}

// one wave per (sequence, query row): keys lane, lane + 64, ... in registers, the head loop inside
template <bool VEC>
__global__ __launch_bounds__(64 * GX_WAVES) void attn_grad_probs_cross_any_kernel(const GradCrossGeo geo) {
  __shared__ __attribute__((aligned(16))) float q_lds[GX_WAVES][GX_MAX_DH];
  __shared__ __attribute__((aligned(16))) float g_lds[GX_WAVES][GX_MAX_DH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * GX_WAVES + wave;  // query token
  if (row >= geo.n_units) return;
  float* qs = q_lds[wave];
  float* gs = g_lds[wave];
  const int Lq = geo.Lq, Lk = geo.Lk, H = geo.H, dh = geo.dh;
  const int64_t d = (int64_t)H * dh;
  const int64_t seq = row / Lq;
  const int i = (int)(row - seq * Lq);
  const int64_t k_base = seq * Lk;
  bool ok[GX_KEYS_PER_LANE];
  float acc[GX_KEYS_PER_LANE];
#pragma unroll
  for (int t = 0; t < GX_KEYS_PER_LANE; ++t) {
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
    float sc[GX_KEYS_PER_LANE], gr[GX_KEYS_PER_LANE];
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < GX_KEYS_PER_LANE; ++t) {
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
    for (int t = 0; t < GX_KEYS_PER_LANE; ++t) {
      sc[t] = sc[t] > -1e29f ? expf(sc[t] - mx) : 0.f;
      sum += sc[t];
    }
    sum = wave_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;  // fully masked row -> zeros
#pragma unroll
    for (int t = 0; t < GX_KEYS_PER_LANE; ++t) acc[t] += ok[t] ? fmaxf(sc[t] * inv * gr[t], 0.f) : 0.f;
  }
  float* const out_row = geo.abar + row * Lk;  // (S, Lq, Lk): row (seq, i)
#pragma unroll
  for (int t = 0; t < GX_KEYS_PER_LANE; ++t)
    if (lane + 64 * t < Lk) out_row[lane + 64 * t] = acc[t] * geo.inv_h;
}

template <int NB>
void launch_grad_cross16(const GradCrossGeo& g, unsigned n_wg, hipStream_t s) {
  hipLaunchKernelGGL((attn_grad_probs_cross16_kernel<NB>), dim3(n_wg), dim3(64 * GX_WAVES), 0, s, g);
}

// ---- joint rollout -----------------------------------------------------------------------------------------------------------------------
constexpr int JR_THREADS = 256;
constexpr int JR_COLS = 16;               // columns of R a workgroup carries through the chain
constexpr int JR_MAX_J = 2 * GX_MAX_L;    // T, A <= 256
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
      float a = old[e];
      const bool top = i < T;
      const float* arow = top ? (map_t ? map_t + (int64_t)i * n_t : nullptr) : map_a + (int64_t)(i - T) * n_a;
      if (arow) {
        const int n = top ? n_t : n_a;
        const float* col = old + (top ? k0_t : k0_a) * CB + j;
        for (int k = 0; k < n; ++k) a = fmaf(arow[k], col[k * CB], a);
      }
      nxt[e] = a;
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

int launch_attn_grad_probs_cross(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* dctx, const uint8_t* kpm, int causal,
                                 int64_t S, int64_t Lq, int64_t Lk, int64_t H, int64_t dh, float* abar, hipStream_t s) {
  if (!q || !k || !v || !dctx || !kpm || !abar) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: null pointer");
  if (Lq < 1 || Lq > GX_MAX_L || Lk < 1 || Lk > GX_MAX_L)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: sequence lengths %lld / %lld unsupported (1 ... %d)", (long long)Lq, (long long)Lk, GX_MAX_L);
  if (dh < 1 || dh > GX_MAX_DH) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: head dim %lld unsupported (1 ... %d)", (long long)dh, GX_MAX_DH);
  if (S < 0 || S > 0x7fffff00LL || H <= 0 || H > 65535 || S * Lq > 0x7fffff00LL || S * Lk > 0x7fffff00LL)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: bad sequence / head count");
  if (causal && Lq != Lk) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: causal needs Lq == Lk (%lld, %lld)", (long long)Lq, (long long)Lk);
  if (ldq < H * dh || ldkv < H * dh || ldq > 0x7fffffffLL || ldkv > 0x7fffffffLL)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: ldq / ldkv must be at least H * dh");
  const bool mfma_shape = dh == GX_DH && Lk <= 64;
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
  g.nqb = (int)nqb;
  g.n_units = mfma ? S * g.nqb : S * Lq;
  const int64_t n_wg = (g.n_units + GX_WAVES - 1) / GX_WAVES;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_grad_probs_cross: too many work items");
  StltProfScope ps(STLT_K_ATTN_PROBS, s);
  stlt_prof_note("attn_grad_probs_cross %s S=%lld Lq=%lld Lk=%lld H=%lld dh=%lld causal=%d", mfma ? "mfma-full" : "generic", (long long)S, (long long)Lq, (long long)Lk,
                 (long long)H, (long long)dh, g.causal);
  stlt_prof_add_bytes((double)S * (Lq + Lk) * H * dh * 4.0 * 2 + (double)S * Lq * Lk * 4.0 + (double)S * Lk);  // q, dctx, k, v, abar, mask
  stlt_prof_note_flops((double)S * H * Lq * Lk * 4.0 * dh * (causal ? 0.5 : 1.0));
  if (mfma) {
    if (nb == 1) launch_grad_cross16<1>(g, (unsigned)n_wg, s);
    else if (nb == 2) launch_grad_cross16<2>(g, (unsigned)n_wg, s);
    else if (nb == 3) launch_grad_cross16<3>(g, (unsigned)n_wg, s);
    else launch_grad_cross16<4>(g, (unsigned)n_wg, s);
    return stlt_check_launch("attn_grad_probs_cross16_kernel");
  }
  const bool vec = dh % 4 == 0 && (ptrs & 15) == 0 && (ldq & 3) == 0 && (ldkv & 3) == 0;  // every q / k / v / dctx slice then starts on 16 bytes
  if (vec) hipLaunchKernelGGL((attn_grad_probs_cross_any_kernel<true>), dim3((unsigned)n_wg), dim3(64 * GX_WAVES), 0, s, g);
  else hipLaunchKernelGGL((attn_grad_probs_cross_any_kernel<false>), dim3((unsigned)n_wg), dim3(64 * GX_WAVES), 0, s, g);
  return stlt_check_launch("attn_grad_probs_cross_any_kernel");
}

int launch_attn_rollout_joint(const float* r_layout, const float* r_appearance, const float* l2a, const float* a2l, const float* f_layout, const float* f_appearance,
                              int64_t n_fusion, int64_t S, int64_t T, int64_t A, float* R, hipStream_t s) {
  if (!R || (n_fusion > 0 && (!l2a || !a2l || !f_layout || !f_appearance))) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: null pointer");
  if (n_fusion < 0 || n_fusion > 64) return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: layer count %lld unsupported (0 ... 64)", (long long)n_fusion);
  if (T < 1 || T > GX_MAX_L || A < 1 || A > GX_MAX_L)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_rollout_joint: token counts %lld / %lld unsupported (1 ... %d)", (long long)T, (long long)A, GX_MAX_L);
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
