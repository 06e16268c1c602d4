// Attention probabilities (include/stlt_hip.h: stlt_attn_probs_fwd, stlt_forward_attention; stlt_attn_probs_cross_fwd,
// stlt_caf_forward_attention): what nn.MultiheadAttention returns with need_weights=True — on the layers of models.py:46-55,118-128 from
// the packed QKV buffer, and on the fusion models' CrossAttentionLayer (reference models.py:362-382, 411-419) with queries in a (S*Lq, ldq)
// buffer and keys in a (S*Lk, ldk) buffer, Lq != Lk in general — per head, or averaged over the heads.  The attention cores keep the
// probabilities in registers between Q·K^T and P·V and the fused kernel never writes Q / K / V; this file is the one place that writes P.
// It has no V and no P·V, and writes S·Lq·Lk (x H) floats.  The packed buffer is the two-buffer case q = qkv, k = qkv + d, ldq = ldk = 3d,
// Lq = Lk = L, and runs on the same kernels.
//
//   MFMA    (dh == 64, Lk <= 64): the 16-row core of attn_rows16.h.
//             sided (any Lq; packed: 16 < L <= 64): a unit = (sequence, 16-row query block) against the NB = ceil(Lk/16) key blocks (causal:
//                                  the blocks up to its own); Lq only sets the number of units; the output row stride is Lk;
//             diag  (packed, L <= 16): a unit = one 16-row block holding P = floor(16/L) whole sequences.
//           The wave loops over the heads itself: per_head stores each head's block, else it accumulates p·(1/H) in registers and stores
//           once — no atomics, no second pass, the same bits on every run.  The next head's fragments are requested as soon as the last
//           MFMA of this head has consumed the registers, so they travel under the softmax and the stores.
//   generic (everything else: any dh <= 256, Lk <= 1024): one wave per (sequence, query row) on the vector ALU in the style of attn_any.hip,
//           lane = key (keys lane, lane + 64, ...: at most 16 per lane, kept in registers), the query row broadcast from LDS, looping over heads.
// Same masks and arithmetic as the cores: masked entries are exactly 0, a row whose keys are all masked is zeros, query rows are not
// filtered by any mask.  Every element of the output is written.
#include <cmath>
#include <cstdint>
#include "common.h"
#include "attn_vec.h"
#include "attn_rows16.h"

namespace {

constexpr int PB_DH = 64;         // head dim of the MFMA path
constexpr int PB_WAVES = 4;       // independent waves per workgroup (both paths)
constexpr int PB_MAX_L = 1024;
constexpr int PB_MAX_DH = 256;
constexpr int PB_KEYS_PER_LANE = PB_MAX_L / 64;

struct ProbsGeo {
  const float* q;      // (S*Lq, ldq), the first H*dh columns
  const float* k;      // (S*Lk, ldk), the first H*dh columns
  const uint8_t* kpm;  // (S*Lk): 1 = padded key
  float* probs;        // (S, Lq, Lk) or (S, H, Lq, Lk)
  int64_t ldq, ldk, n_units;
  int Lq, Lk, H, dh;
  int nqb;             // sided: query blocks per sequence
  int P, n_tokens;     // diag: sequences per 16-row block, S * L (read by DiagRows alone: the sided and vector kernels ignore both)
  int causal, per_head;
  float scale, inv_h;
};

template <int NB, class Rows>
__global__ __launch_bounds__(64 * PB_WAVES) void attn_probs16_kernel(const ProbsGeo geo) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * PB_WAVES + wave;
  if (unit >= geo.n_units) return;  // wave-uniform: no lane of a working wave is ever switched off
  const int H = geo.H;
  const bool causal = geo.causal != 0;
  const Rows rows(geo, unit);
  const int q_local = rows.qb * 16 + li;
  const Keys16<NB> keys(rows, q_local, lg, geo.kpm, causal);

  f32x4 kf[NB][4], qc[4];
  auto load_head = [&](int head) __attribute__((always_inline)) {
    const int col = head * PB_DH + 4 * lg;
    load_frag16(qc, geo.q + q_read(rows, q_local) * geo.ldq + col);
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
      if (rows.used(kb, causal)) load_frag16(kf[kb], geo.k + k_read(rows, kb * 16 + li) * geo.ldk + col);
  };

  // where this lane's values go: the query's row of its sequence's (Lq, Lk) map
  const int64_t seq = rows.out_seq(keys.q_seq);
  const int64_t map = (int64_t)geo.Lq * geo.Lk;
  float* const out_row = geo.probs + (geo.per_head ? seq * H : seq) * map + (int64_t)keys.q_pos * geo.Lk;

  f32x4 acc[NB];
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
  load_head(0);
  for (int head = 0; head < H; ++head) {
    f32x4 st[NB];  // st[kb][r] = score of key kb*16 + 4*lg + r against query q_local
    scores16<NB>(rows, causal, kf, qc, st);
    if (head + 1 < H) load_head(head + 1);  // the fragment registers are dead: the next head's loads go under the softmax and the stores
    const float inv = softmax16<NB>(st, keys.ok, geo.scale);
    if (geo.per_head) {
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) st[kb] = st[kb] * inv;
      store_row16<NB>(out_row + head * map, st, keys);
    } else {
      const float w = inv * geo.inv_h;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) acc[kb] += st[kb] * w;
    }
  }
  if (!geo.per_head) store_row16<NB>(out_row, acc, keys);
}

// one wave per (sequence, query row): keys lane, lane + 64, ... in registers, the head loop inside
template <bool VEC>
__global__ __launch_bounds__(64 * PB_WAVES) void attn_probs_any_kernel(const ProbsGeo geo) {
  __shared__ __attribute__((aligned(16))) float q_lds[PB_WAVES][PB_MAX_DH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * PB_WAVES + wave;  // query token
  if (row >= geo.n_units) return;
  float* qs = q_lds[wave];
  const int Lq = geo.Lq, Lk = geo.Lk, H = geo.H, dh = geo.dh;
  const int64_t seq = row / Lq;
  const int i = (int)(row - seq * Lq);
  const int64_t k_base = seq * Lk;
  bool ok[PB_KEYS_PER_LANE];
  float acc[PB_KEYS_PER_LANE];
#pragma unroll
  for (int t = 0; t < PB_KEYS_PER_LANE; ++t) {
    const int j = lane + 64 * t;
    ok[t] = j < Lk && geo.kpm[k_base + (j < Lk ? j : 0)] == 0 && (!geo.causal || j <= i);
    acc[t] = 0.f;
  }
  const int64_t map = (int64_t)Lq * Lk;
  float* const out_row = geo.probs + (geo.per_head ? seq * H : seq) * map + (int64_t)i * Lk;
  for (int head = 0; head < H; ++head) {
    const float* qrow = geo.q + row * geo.ldq + (int64_t)head * dh;
    wave_lds_sync();  // the previous head's reads of qs are done
    for (int c = lane; c < dh; c += 64) qs[c] = qrow[c];
    wave_lds_sync();
    float sc[PB_KEYS_PER_LANE];
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < PB_KEYS_PER_LANE; ++t) {
      sc[t] = -1e30f;
      if (64 * t < Lk) {  // wave-uniform
        if (ok[t]) sc[t] = dot_row<VEC>(qs, geo.k + (k_base + lane + 64 * t) * geo.ldk + (int64_t)head * dh, dh) * geo.scale;
        mx = fmaxf(mx, sc[t]);
      }
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < PB_KEYS_PER_LANE; ++t) {
      sc[t] = sc[t] > -1e29f ? expf(sc[t] - mx) : 0.f;
      sum += sc[t];
    }
    sum = wave_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;  // fully masked row -> zeros
    if (geo.per_head) {
#pragma unroll
      for (int t = 0; t < PB_KEYS_PER_LANE; ++t)
        if (lane + 64 * t < Lk) out_row[head * map + lane + 64 * t] = sc[t] * inv;
    } else {
      const float w = inv * geo.inv_h;
#pragma unroll
      for (int t = 0; t < PB_KEYS_PER_LANE; ++t) acc[t] += sc[t] * w;
    }
  }
  if (!geo.per_head) {
#pragma unroll
    for (int t = 0; t < PB_KEYS_PER_LANE; ++t)
      if (lane + 64 * t < Lk) out_row[lane + 64 * t] = acc[t];
  }
}

// what both launchers share once their checks have passed: the two sides, the masks and the head weights
ProbsGeo probs_geo(const float* q, int64_t ldq, const float* k, int64_t ldk, const uint8_t* kpm, int causal, int64_t S, int64_t Lq, int64_t Lk, int64_t H,
                   int64_t dh, int per_head, float* probs) {
  ProbsGeo g;
  g.q = q; g.k = k; g.kpm = kpm; g.probs = probs; g.ldq = ldq; g.ldk = ldk;
  g.Lq = (int)Lq; g.Lk = (int)Lk; g.H = (int)H; g.dh = (int)dh;
  g.nqb = (int)((Lq + 15) / 16); g.P = 1; g.n_tokens = (int)(S * Lk);
  g.causal = causal ? 1 : 0; g.per_head = per_head;
  g.scale = 1.0f / sqrtf((float)dh);
  g.inv_h = 1.0f / (float)H;
  return g;
}

template <int NB, class Rows>
void launch_probs16(const ProbsGeo& g, unsigned n_wg, hipStream_t s) {
  hipLaunchKernelGGL((attn_probs16_kernel<NB, Rows>), dim3(n_wg), dim3(64 * PB_WAVES), 0, s, g);
}

// the sided MFMA kernel for nb key blocks / the vector kernel (vec: every q / k slice of a row starts on 16 bytes)
void launch_probs_sided(const ProbsGeo& g, int nb, unsigned n_wg, hipStream_t s) {
  if (nb == 1) launch_probs16<1, SidedRows>(g, n_wg, s);
  else if (nb == 2) launch_probs16<2, SidedRows>(g, n_wg, s);
  else if (nb == 3) launch_probs16<3, SidedRows>(g, n_wg, s);
  else launch_probs16<4, SidedRows>(g, n_wg, s);
}
void launch_probs_any(const ProbsGeo& g, bool vec, unsigned n_wg, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((attn_probs_any_kernel<true>), dim3(n_wg), dim3(64 * PB_WAVES), 0, s, g);
  else hipLaunchKernelGGL((attn_probs_any_kernel<false>), dim3(n_wg), dim3(64 * PB_WAVES), 0, s, g);
}

}  // namespace

int launch_attn_probs(const float* qkv, const uint8_t* kpm, int causal, int64_t S, int64_t L, int64_t H, int64_t dh, int per_head, float* probs,
                      hipStream_t s) {
  if (!qkv || !kpm || !probs) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: null pointer");
  if (L < 1 || L > PB_MAX_L) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: sequence length %lld unsupported (1 ... %d)", (long long)L, PB_MAX_L);
  if (dh < 1 || dh > PB_MAX_DH) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: head dim %lld unsupported (1 ... %d)", (long long)dh, PB_MAX_DH);
  if (S < 0 || S > 0x7fffff00LL || H <= 0 || H > 65535 || S * L > 0x7fffff00LL) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: bad sequence / head count");
  if (per_head != 0 && per_head != 1) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: per_head must be 0 or 1");
  if (dh == PB_DH && ((uintptr_t)qkv & 15)) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: qkv must be 16-byte aligned");
  if ((uintptr_t)qkv & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: qkv must be 4-byte aligned");
  if ((uintptr_t)probs & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: probs must be 4-byte aligned");
  if (S == 0) return 0;
  const int64_t d = H * dh;
  ProbsGeo g = probs_geo(qkv, 3 * d, qkv + d, 3 * d, kpm, causal, S, L, L, H, dh, per_head, probs);
  const bool mfma = dh == PB_DH && L <= 64;
  if (mfma && L <= 16) {
    g.P = (int)(16 / L);
    g.n_units = (S + g.P - 1) / g.P;
  } else {
    g.n_units = mfma ? S * g.nqb : S * L;
  }
  const int64_t n_wg = (g.n_units + PB_WAVES - 1) / PB_WAVES;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: too many work items");
  StltProfScope ps(STLT_K_ATTN_PROBS, s);
  stlt_prof_note("attn_probs %s S=%lld L=%lld H=%lld dh=%lld causal=%d per_head=%d", mfma ? (L <= 16 ? "mfma-diag" : "mfma-full") : "generic", (long long)S,
                 (long long)L, (long long)H, (long long)dh, g.causal, per_head);
  stlt_prof_add_bytes((double)S * L * H * dh * 4.0 * 2 + (double)S * L * L * 4.0 * (per_head ? (double)H : 1.0) + (double)S * L);  // q, k, probs, mask
  stlt_prof_note_flops((double)S * H * L * L * 2.0 * dh * (causal ? 0.5 : 1.0));
  if (mfma) {
    if (L <= 16) launch_probs16<1, DiagRows>(g, (unsigned)n_wg, s);
    else launch_probs_sided(g, g.nqb, (unsigned)n_wg, s);
    return stlt_check_launch("attn_probs16_kernel");
  }
  launch_probs_any(g, dh % 4 == 0 && ((uintptr_t)qkv & 15) == 0, (unsigned)n_wg, s);  // every q / k slice of a packed row then starts on 16 bytes
  return stlt_check_launch("attn_probs_any_kernel");
}

int launch_attn_probs_cross(const float* q, int64_t ldq, const float* k, int64_t ldk, const uint8_t* kpm, int causal, int64_t S, int64_t Lq,
                            int64_t Lk, int64_t H, int64_t dh, int per_head, float* probs, hipStream_t s) {
  if (!q || !k || !kpm || !probs) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: null pointer");
  if (Lq < 1 || Lq > PB_MAX_L || Lk < 1 || Lk > PB_MAX_L)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: sequence lengths %lld / %lld unsupported (1 ... %d)", (long long)Lq, (long long)Lk, PB_MAX_L);
  if (dh < 1 || dh > PB_MAX_DH) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: head dim %lld unsupported (1 ... %d)", (long long)dh, PB_MAX_DH);
  if (S < 0 || S > 0x7fffff00LL || H <= 0 || H > 65535 || S * Lq > 0x7fffff00LL || S * Lk > 0x7fffff00LL)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: bad sequence / head count");
  if (per_head != 0 && per_head != 1) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: per_head must be 0 or 1");
  if (causal && Lq != Lk) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: causal needs Lq == Lk (%lld, %lld)", (long long)Lq, (long long)Lk);
  if (ldq < H * dh || ldk < H * dh || ldq > 0x7fffffffLL || ldk > 0x7fffffffLL)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: ldq / ldk must be at least H * dh");
  const bool mfma_shape = dh == PB_DH && Lk <= 64;
#ifdef STLT_PROBS_CROSS_NO_MFMA  // the A/B build of tools/bench_fusion_attention.py (build.variant): every shape on the vector-ALU kernel,
  const bool mfma = false;       // the header's contract (alignment refusals included) unchanged
#else
  const bool mfma = mfma_shape;
#endif
  if (mfma_shape && ((((uintptr_t)q | (uintptr_t)k) & 15) || (ldq & 3) || (ldk & 3)))
    return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: q and k must be 16-byte aligned and ldq, ldk multiples of 4 at head dim 64 with Lk <= 64");
  if (((uintptr_t)q | (uintptr_t)k) & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: q and k must be 4-byte aligned");
  if ((uintptr_t)probs & 3) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: probs must be 4-byte aligned");
  if (S == 0) return 0;
  ProbsGeo g = probs_geo(q, ldq, k, ldk, kpm, causal, S, Lq, Lk, H, dh, per_head, probs);
  g.n_units = mfma ? S * g.nqb : S * Lq;
  const int64_t n_wg = (g.n_units + PB_WAVES - 1) / PB_WAVES;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: too many work items");
  StltProfScope ps(STLT_K_ATTN_PROBS, s);
  stlt_prof_note("attn_probs_cross %s S=%lld Lq=%lld Lk=%lld H=%lld dh=%lld causal=%d per_head=%d", mfma ? "mfma-full" : "generic", (long long)S, (long long)Lq,
                 (long long)Lk, (long long)H, (long long)dh, g.causal, per_head);
  stlt_prof_add_bytes((double)S * (Lq + Lk) * H * dh * 4.0 + (double)S * Lq * Lk * 4.0 * (per_head ? (double)H : 1.0) + (double)S * Lk);  // q, k, probs, mask
  stlt_prof_note_flops((double)S * H * Lq * Lk * 2.0 * dh * (causal ? 0.5 : 1.0));
  if (mfma) {
    launch_probs_sided(g, (int)((Lk + 15) / 16), (unsigned)n_wg, s);
    return stlt_check_launch("attn_probs16_kernel");
  }
  launch_probs_any(g, dh % 4 == 0 && (((uintptr_t)q | (uintptr_t)k) & 15) == 0 && (ldq & 3) == 0 && (ldk & 3) == 0, (unsigned)n_wg, s);  // every q / k slice then starts on 16 bytes
  return stlt_check_launch("attn_probs_any_kernel");
}
