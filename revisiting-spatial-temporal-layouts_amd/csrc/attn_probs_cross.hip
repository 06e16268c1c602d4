// Attention probabilities with queries and keys from different buffers (include/stlt_hip.h: stlt_attn_probs_cross_fwd,
// stlt_caf_forward_attention): what the nn.MultiheadAttention of the fusion models' CrossAttentionLayer (reference models.py:362-382,
// 411-419) returns with need_weights=True — stlt_attn_cross_fwd without its value half.  Queries lie in a (S*Lq, ldq) buffer, keys in a
// (S*Lk, ldk) buffer, Lq != Lk in general; the output is (S, Lq, Lk) averaged over the heads, or (S, H, Lq, Lk).
//
//   MFMA    (dh == 64, Lk <= 64, any Lq): the FULL form of attn_probs.hip's attn_probs16_kernel.  A unit = (sequence, 16-row query block)
//           against the NB = ceil(Lk/16) key blocks; S^T = K·Q^T on v_mfma_f32_16x16x4_f32 with swapped operands, a row's maximum and sum
//           from the two lane-group exchanges of wave_dpp.h, fragments straight from global memory, no LDS, the next head's loads issued
//           once the last MFMA of this head has consumed the registers.  What differs from the packed kernel: the query side and the key
//           side have their own row -> token maps, each with its own spare token for absent rows; Lq only sets the number of units; the
//           output row stride is Lk.
//   generic (everything else: any dh <= 256, Lk <= 1024): one wave per (sequence, query row) on the vector ALU, lane = key (keys lane,
//           lane + 64, ...), the query row broadcast from LDS, looping over the heads — attn_probs_any_kernel with two buffers.
// Same masks and arithmetic as the cores: masked entries are exactly 0, a row whose keys are all masked is zeros, query rows are not
// filtered by any mask.  Every element of the output is written.  The head average is summed head by head in registers: no atomics.
#include <cmath>
#include <cstdint>
#include "common.h"
#include "attn_vec.h"
#include "wave_dpp.h"

namespace {

constexpr int PX_DH = 64;         // head dim of the MFMA path
constexpr int PX_WAVES = 4;       // independent waves per workgroup (both paths)
constexpr int PX_MAX_L = 1024;
constexpr int PX_MAX_DH = 256;
constexpr int PX_KEYS_PER_LANE = PX_MAX_L / 64;

struct CrossGeo {
  const float* q;      // (S*Lq, ldq), the first H*dh columns
  const float* k;      // (S*Lk, ldk), the first H*dh columns
  const uint8_t* kpm;  // (S*Lk): 1 = padded key
  float* probs;        // (S, Lq, Lk) or (S, H, Lq, Lk)
  int64_t ldq, ldk, n_units;
  int S, Lq, Lk, H, dh, nqb;  // nqb = query blocks per sequence (MFMA)
  int causal, per_head;
  float scale, inv_h;
};

template <int NB>
__global__ __launch_bounds__(64 * PX_WAVES) void attn_probs_cross16_kernel(const CrossGeo geo) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * PX_WAVES + wave;
  if (unit >= geo.n_units) return;  // wave-uniform: no lane of a working wave is ever switched off
  const int H = geo.H, Lq = geo.Lq, Lk = geo.Lk;
  const bool causal = geo.causal != 0;

  const int64_t seq = unit / geo.nqb;
  const int qb = (int)(unit - seq * geo.nqb);
  const int64_t q0 = seq * Lq, k0 = seq * Lk;  // the sequence's first query / key token
  // local row -> token of each side, -1 = no such row; absent rows read the side's spare token (they are masked / never stored)
  auto q_token = [&](int local) __attribute__((always_inline)) -> int64_t { return local < Lq ? q0 + local : -1; };
  auto k_token = [&](int local) __attribute__((always_inline)) -> int64_t { return local < Lk ? k0 + local : -1; };
  const int64_t q_spare = q0 + Lq - 1, k_spare = k0 + Lk - 1;
  auto used = [&](int kb) __attribute__((always_inline)) { return !causal || kb <= qb; };  // causal: Lq == Lk

  // the query of this lane's column and the four keys of its rows in every key block: position, validity, padding
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

  f32x4 kf[NB][4], qc[4];
  auto load_head = [&](int head) __attribute__((always_inline)) {
    const int col = head * PX_DH + 4 * lg;
    const float* qrow = geo.q + (q_tok >= 0 ? q_tok : q_spare) * geo.ldq + col;
#pragma unroll
    for (int c = 0; c < 4; ++c) qc[c] = *reinterpret_cast<const f32x4*>(qrow + 16 * c);
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      if (!used(kb)) continue;
      const int64_t tok = k_token(kb * 16 + li);
      const float* krow = geo.k + (tok >= 0 ? tok : k_spare) * geo.ldk + col;
#pragma unroll
      for (int c = 0; c < 4; ++c) kf[kb][c] = *reinterpret_cast<const f32x4*>(krow + 16 * c);
    }
  };

  // where this lane's values go: row q_pos of its sequence's (Lq, Lk) map
  const int64_t map = (int64_t)Lq * Lk;
  float* const out_row = geo.probs + (geo.per_head ? seq * H : seq) * map + (int64_t)q_pos * Lk;
  auto store = [&](float* dst, const f32x4 (&p)[NB]) __attribute__((always_inline)) {
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (k_col[kb][r]) dst[k_pos[kb][r]] = p[kb][r];
  };

  f32x4 acc[NB];
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
  load_head(0);
  for (int head = 0; head < H; ++head) {
    // ---- S^T blocks: st[kb][r] = score of key kb*16 + 4*lg + r against query qb*16 + li
    f32x4 st[NB];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      st[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (used(kb)) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) st[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][c][e], qc[c][e], st[kb], 0, 0, 0);
      }
    }
    if (head + 1 < H) load_head(head + 1);  // the fragment registers are dead: the next head's loads go under the softmax and the stores
    // ---- mask + softmax (a query's scores: 4 per key block, over the 4 lanes lg = 0..3)
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
    if (geo.per_head) {
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) st[kb] = st[kb] * inv;
      store(out_row + head * map, st);
    } else {
      const float w = inv * geo.inv_h;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) acc[kb] += st[kb] * w;
    }
  }
  if (!geo.per_head) store(out_row, acc);
}

// one wave per (sequence, query row): keys lane, lane + 64, ... in registers, the head loop inside
template <bool VEC>
__global__ __launch_bounds__(64 * PX_WAVES) void attn_probs_cross_any_kernel(const CrossGeo geo) {
  __shared__ __attribute__((aligned(16))) float q_lds[PX_WAVES][PX_MAX_DH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * PX_WAVES + wave;  // query token
  if (row >= geo.n_units) return;
  float* qs = q_lds[wave];
  const int Lq = geo.Lq, Lk = geo.Lk, H = geo.H, dh = geo.dh;
  const int64_t seq = row / Lq;
  const int i = (int)(row - seq * Lq);
  const int64_t k_base = seq * Lk;
  bool ok[PX_KEYS_PER_LANE];
  float acc[PX_KEYS_PER_LANE];
#pragma unroll
  for (int t = 0; t < PX_KEYS_PER_LANE; ++t) {
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
    float sc[PX_KEYS_PER_LANE];
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < PX_KEYS_PER_LANE; ++t) {
      sc[t] = -1e30f;
      if (64 * t < Lk) {  // wave-uniform
        if (ok[t]) sc[t] = dot_row<VEC>(qs, geo.k + (k_base + lane + 64 * t) * geo.ldk + (int64_t)head * dh, dh) * geo.scale;
        mx = fmaxf(mx, sc[t]);
      }
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < PX_KEYS_PER_LANE; ++t) {
      sc[t] = sc[t] > -1e29f ? expf(sc[t] - mx) : 0.f;
      sum += sc[t];
    }
    sum = wave_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;  // fully masked row -> zeros
    if (geo.per_head) {
#pragma unroll
      for (int t = 0; t < PX_KEYS_PER_LANE; ++t)
        if (lane + 64 * t < Lk) out_row[head * map + lane + 64 * t] = sc[t] * inv;
    } else {
      const float w = inv * geo.inv_h;
#pragma unroll
      for (int t = 0; t < PX_KEYS_PER_LANE; ++t) acc[t] += sc[t] * w;
    }
  }
  if (!geo.per_head) {
#pragma unroll
    for (int t = 0; t < PX_KEYS_PER_LANE; ++t)
      if (lane + 64 * t < Lk) out_row[lane + 64 * t] = acc[t];
  }
}

template <int NB>
void launch_cross16(const CrossGeo& g, unsigned n_wg, hipStream_t s) {
  hipLaunchKernelGGL((attn_probs_cross16_kernel<NB>), dim3(n_wg), dim3(64 * PX_WAVES), 0, s, g);
}

}  // namespace

int launch_attn_probs_cross(const float* q, int64_t ldq, const float* k, int64_t ldk, const uint8_t* kpm, int causal, int64_t S, int64_t Lq,
                            int64_t Lk, int64_t H, int64_t dh, int per_head, float* probs, hipStream_t s) {
  if (!q || !k || !kpm || !probs) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: null pointer");
  if (Lq < 1 || Lq > PX_MAX_L || Lk < 1 || Lk > PX_MAX_L)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: sequence lengths %lld / %lld unsupported (1 ... %d)", (long long)Lq, (long long)Lk, PX_MAX_L);
  if (dh < 1 || dh > PX_MAX_DH) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: head dim %lld unsupported (1 ... %d)", (long long)dh, PX_MAX_DH);
  if (S < 0 || S > 0x7fffff00LL || H <= 0 || H > 65535 || S * Lq > 0x7fffff00LL || S * Lk > 0x7fffff00LL)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: bad sequence / head count");
  if (per_head != 0 && per_head != 1) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: per_head must be 0 or 1");
  if (causal && Lq != Lk) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: causal needs Lq == Lk (%lld, %lld)", (long long)Lq, (long long)Lk);
  if (ldq < H * dh || ldk < H * dh || ldq > 0x7fffffffLL || ldk > 0x7fffffffLL)
    return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: ldq / ldk must be at least H * dh");
  const bool mfma_shape = dh == PX_DH && Lk <= 64;
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
  CrossGeo g;
  g.q = q; g.k = k; g.kpm = kpm; g.probs = probs; g.ldq = ldq; g.ldk = ldk;
  g.S = (int)S; g.Lq = (int)Lq; g.Lk = (int)Lk; g.H = (int)H; g.dh = (int)dh;
  g.causal = causal ? 1 : 0; g.per_head = per_head;
  g.scale = 1.0f / sqrtf((float)dh);
  g.inv_h = 1.0f / (float)H;
  g.nqb = (int)((Lq + 15) / 16);
  const int nb = (int)((Lk + 15) / 16);
  g.n_units = mfma ? S * g.nqb : S * Lq;
  const int64_t n_wg = (g.n_units + PX_WAVES - 1) / PX_WAVES;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_cross_fwd: too many work items");
  StltProfScope ps(STLT_K_ATTN_PROBS, s);
  stlt_prof_note("attn_probs_cross %s S=%lld Lq=%lld Lk=%lld H=%lld dh=%lld causal=%d per_head=%d", mfma ? "mfma-full" : "generic", (long long)S, (long long)Lq,
                 (long long)Lk, (long long)H, (long long)dh, g.causal, per_head);
  stlt_prof_add_bytes((double)S * (Lq + Lk) * H * dh * 4.0 + (double)S * Lq * Lk * 4.0 * (per_head ? (double)H : 1.0) + (double)S * Lk);  // q, k, probs, mask
  stlt_prof_note_flops((double)S * H * Lq * Lk * 2.0 * dh * (causal ? 0.5 : 1.0));
  if (mfma) {
    if (nb == 1) launch_cross16<1>(g, (unsigned)n_wg, s);
    else if (nb == 2) launch_cross16<2>(g, (unsigned)n_wg, s);
    else if (nb == 3) launch_cross16<3>(g, (unsigned)n_wg, s);
    else launch_cross16<4>(g, (unsigned)n_wg, s);
    return stlt_check_launch("attn_probs_cross16_kernel");
  }
  const bool vec = dh % 4 == 0 && (((uintptr_t)q | (uintptr_t)k) & 15) == 0 && (ldq & 3) == 0 && (ldk & 3) == 0;  // every q / k slice then starts on 16 bytes
  if (vec) hipLaunchKernelGGL((attn_probs_cross_any_kernel<true>), dim3((unsigned)n_wg), dim3(64 * PX_WAVES), 0, s, g);
  else hipLaunchKernelGGL((attn_probs_cross_any_kernel<false>), dim3((unsigned)n_wg), dim3(64 * PX_WAVES), 0, s, g);
  return stlt_check_launch("attn_probs_cross_any_kernel");
}
