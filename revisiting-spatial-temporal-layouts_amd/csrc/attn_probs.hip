// Attention probabilities of K3 (include/stlt_hip.h: stlt_attn_probs_fwd, stlt_forward_attention): what nn.MultiheadAttention returns
// with need_weights=True on the layers of models.py:46-55,118-128 — per head, or averaged over the heads.  The attention cores keep the
// probabilities in registers between Q·K^T and P·V and the fused kernel never writes Q / K / V; this file is the one place that writes P.
// It reads two of the three projections of the packed QKV buffer, has no V and no P·V, and writes S·L·L (x H) floats.
//
//   MFMA    (dh == 64, L <= 64): attn16.hip's dataflow without its value half.  S^T = K·Q^T on v_mfma_f32_16x16x4_f32 with swapped
//           operands: lane (li, lg) holds, for query row li of a 16-row block, the scores of keys 4 lg .. 4 lg + 3 of every key block, so a
//           row's maximum and sum are in-register plus two exchanges between the four lane groups.  Q and K fragments come straight from
//           global memory in operand shape; there is no LDS at all (each lane reads the padding bytes of its own four keys).
//             FULL (16 < L <= 64): a unit = (sequence, query block) against the NB = ceil(L/16) key blocks (causal: the blocks up to its own);
//             DIAG (L <= 16)     : a unit = one 16-row block holding P = floor(16/L) whole sequences; pairs of different sequences are masked
//                                  off and have no place in the output.
//           The wave loops over the heads itself: per_head stores each head's block, else it accumulates p·(1/H) in registers and stores
//           once — no atomics, no second pass, the same bits on every run.  The next head's fragments are requested as soon as the last
//           MFMA of this head has consumed the registers, so they travel under the softmax and the stores.  Stores are four-byte accesses
//           (a row of L floats is not 16-byte aligned for L = 7).
//   generic (everything else: any dh <= 256, L <= 1024): one wave per (sequence, query row) on the vector ALU in the style of attn_any.hip,
//           lane = key (keys lane, lane + 64, ...: at most 16 per lane, kept in registers), the query row broadcast from LDS, looping over heads.
// Same masks and arithmetic as the cores: masked entries are exactly 0, a row whose keys are all masked is zeros, query rows are not
// filtered by the padding mask.  Every element of the output is written.
#include <cmath>
#include <cstdint>
#include "common.h"
#include "attn_vec.h"
#include "wave_dpp.h"

namespace {

constexpr int PB_DH = 64;         // head dim of the MFMA path
constexpr int PB_WAVES = 4;       // independent waves per workgroup (both paths)
constexpr int PB_MAX_L = 1024;
constexpr int PB_MAX_DH = 256;
constexpr int PB_KEYS_PER_LANE = PB_MAX_L / 64;

struct ProbsGeo {
  const float* qkv;    // packed (S*L, 3*H*dh): q | k | v
  const uint8_t* kpm;  // one byte per token: 1 = padded key
  float* probs;        // (S, L, L) or (S, H, L, L)
  int64_t n_units;
  int n_tokens, S, L, H, dh, P;  // P = sequences per 16-row block (DIAG), 1 for FULL
  int causal, per_head;
  float scale, inv_h;
};

template <int NB, bool FULL>
__global__ __launch_bounds__(64 * PB_WAVES) void attn_probs16_kernel(const ProbsGeo geo) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * PB_WAVES + wave;
  if (unit >= geo.n_units) return;  // wave-uniform: no lane of a working wave is ever switched off
  const int H = geo.H, L = geo.L, d = H * PB_DH;
  const int64_t ld = 3 * (int64_t)d;
  const bool causal = geo.causal != 0;

  // FULL: the unit's sequence and query block; DIAG: its block of P whole sequences
  const int64_t item = FULL ? unit / NB : unit;
  const int qb = FULL ? (int)(unit - item * NB) : 0;
  const int rows = FULL ? L : geo.P * L;                                   // rows of the item
  const int64_t t0 = FULL ? item * L : item * (int64_t)rows;               // its first token
  // local row of the item -> token, -1 = no such row
  auto row_token = [&](int local) __attribute__((always_inline)) -> int64_t {
    return (local < rows && t0 + local < geo.n_tokens) ? t0 + local : -1;
  };
  int64_t spare = t0 + rows - 1;  // a valid token to read in place of an absent row (such rows are masked / never stored)
  if (spare > geo.n_tokens - 1) spare = geo.n_tokens - 1;
  auto used = [&](int kb) __attribute__((always_inline)) { return !FULL || !causal || kb <= qb; };

  // the query of this lane's column and the four keys of its rows in every key block: (sequence in block, position), validity, padding
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

  f32x4 kf[NB][4], qc[4];
  auto load_head = [&](int head) __attribute__((always_inline)) {
    const float* base = geo.qkv + head * PB_DH + 4 * lg;
    const float* qrow = base + (q_tok >= 0 ? q_tok : spare) * ld;
#pragma unroll
    for (int c = 0; c < 4; ++c) qc[c] = *reinterpret_cast<const f32x4*>(qrow + 16 * c);
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      if (!used(kb)) continue;
      const int64_t tok = row_token(kb * 16 + li);
      const float* krow = base + d + (tok >= 0 ? tok : spare) * ld;
#pragma unroll
      for (int c = 0; c < 4; ++c) kf[kb][c] = *reinterpret_cast<const f32x4*>(krow + 16 * c);
    }
  };

  // where this lane's values go: row q_pos of its sequence's (L, L) map
  const int64_t seq = FULL ? item : item * geo.P + q_seq;
  const int64_t map = (int64_t)L * L;
  float* const out_row = geo.probs + (geo.per_head ? seq * H : seq) * map + (int64_t)q_pos * L;
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
__global__ __launch_bounds__(64 * PB_WAVES) void attn_probs_any_kernel(const ProbsGeo geo) {
  __shared__ __attribute__((aligned(16))) float q_lds[PB_WAVES][PB_MAX_DH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * PB_WAVES + wave;  // query token
  if (row >= geo.n_units) return;
  float* qs = q_lds[wave];
  const int L = geo.L, H = geo.H, dh = geo.dh;
  const int64_t d = (int64_t)H * dh, ld = 3 * d;
  const int64_t seq = row / L;
  const int i = (int)(row - seq * L);
  const int64_t k_base = seq * L;
  bool ok[PB_KEYS_PER_LANE];
  float acc[PB_KEYS_PER_LANE];
#pragma unroll
  for (int t = 0; t < PB_KEYS_PER_LANE; ++t) {
    const int j = lane + 64 * t;
    ok[t] = j < L && geo.kpm[k_base + (j < L ? j : 0)] == 0 && (!geo.causal || j <= i);
    acc[t] = 0.f;
  }
  const int64_t map = (int64_t)L * L;
  float* const out_row = geo.probs + (geo.per_head ? seq * H : seq) * map + (int64_t)i * L;
  for (int head = 0; head < H; ++head) {
    const float* qrow = geo.qkv + row * ld + (int64_t)head * dh;
    wave_lds_sync();  // the previous head's reads of qs are done
    for (int c = lane; c < dh; c += 64) qs[c] = qrow[c];
    wave_lds_sync();
    float sc[PB_KEYS_PER_LANE];
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < PB_KEYS_PER_LANE; ++t) {
      sc[t] = -1e30f;
      if (64 * t < L) {  // wave-uniform
        if (ok[t]) sc[t] = dot_row<VEC>(qs, geo.qkv + (k_base + lane + 64 * t) * ld + d + (int64_t)head * dh, dh) * geo.scale;
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
        if (lane + 64 * t < L) out_row[head * map + lane + 64 * t] = sc[t] * inv;
    } else {
      const float w = inv * geo.inv_h;
#pragma unroll
      for (int t = 0; t < PB_KEYS_PER_LANE; ++t) acc[t] += sc[t] * w;
    }
  }
  if (!geo.per_head) {
#pragma unroll
    for (int t = 0; t < PB_KEYS_PER_LANE; ++t)
      if (lane + 64 * t < L) out_row[lane + 64 * t] = acc[t];
  }
}

template <int NB, bool FULL>
void launch_probs16(const ProbsGeo& g, unsigned n_wg, hipStream_t s) {
  hipLaunchKernelGGL((attn_probs16_kernel<NB, FULL>), dim3(n_wg), dim3(64 * PB_WAVES), 0, s, g);
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
  ProbsGeo g;
  g.qkv = qkv; g.kpm = kpm; g.probs = probs;
  g.n_tokens = (int)(S * L); g.S = (int)S; g.L = (int)L; g.H = (int)H; g.dh = (int)dh; g.P = 1;
  g.causal = causal ? 1 : 0; g.per_head = per_head;
  g.scale = 1.0f / sqrtf((float)dh);
  g.inv_h = 1.0f / (float)H;
  const bool mfma = dh == PB_DH && L <= 64;
  int nb = 1;
  if (mfma && L <= 16) {
    g.P = (int)(16 / L);
    g.n_units = (S + g.P - 1) / g.P;
  } else if (mfma) {
    nb = (int)((L + 15) / 16);
    g.n_units = S * nb;
  } else {
    g.n_units = S * L;
  }
  const int64_t n_wg = (g.n_units + PB_WAVES - 1) / PB_WAVES;
  if (n_wg > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_probs_fwd: too many work items");
  StltProfScope ps(STLT_K_ATTN_PROBS, s);
  stlt_prof_note("attn_probs %s S=%lld L=%lld H=%lld dh=%lld causal=%d per_head=%d", mfma ? (L <= 16 ? "mfma-diag" : "mfma-full") : "generic", (long long)S,
                 (long long)L, (long long)H, (long long)dh, g.causal, per_head);
  stlt_prof_add_bytes((double)S * L * H * dh * 4.0 * 2 + (double)S * L * L * 4.0 * (per_head ? (double)H : 1.0) + (double)S * L);  // q, k, probs, mask
  stlt_prof_note_flops((double)S * H * L * L * 2.0 * dh * (causal ? 0.5 : 1.0));
  if (mfma) {
    if (L <= 16) launch_probs16<1, false>(g, (unsigned)n_wg, s);
    else if (nb == 2) launch_probs16<2, true>(g, (unsigned)n_wg, s);
    else if (nb == 3) launch_probs16<3, true>(g, (unsigned)n_wg, s);
    else launch_probs16<4, true>(g, (unsigned)n_wg, s);
    return stlt_check_launch("attn_probs16_kernel");
  }
  const bool vec = dh % 4 == 0 && ((uintptr_t)qkv & 15) == 0;  // every q / k slice of a packed row then starts on 16 bytes
  if (vec) hipLaunchKernelGGL((attn_probs_any_kernel<true>), dim3((unsigned)n_wg), dim3(64 * PB_WAVES), 0, s, g);
  else hipLaunchKernelGGL((attn_probs_any_kernel<false>), dim3((unsigned)n_wg), dim3(64 * PB_WAVES), 0, s, g);
  return stlt_check_launch("attn_probs_any_kernel");
}
