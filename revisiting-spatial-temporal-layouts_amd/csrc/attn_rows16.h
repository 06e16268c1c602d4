// The 16-row score / softmax core of the attention-map kernels (attn_probs.hip: attn_probs16_kernel, attn_grad_probs.hip:
// attn_grad_probs16_kernel): attn16.hip's dataflow without its P·V half, head dim 64, at most 64 keys.  One wave owns a unit of 16 query
// rows against NB blocks of 16 keys.  S^T = K·Q^T on v_mfma_f32_16x16x4_f32 with swapped operands: lane (li, lg) holds, for query row li
// of the unit, the scores of keys 4 lg .. 4 lg + 3 of every key block, so a row's maximum and sum are in-register plus two exchanges
// between the four lane groups (wave_dpp.h).  Fragments come straight from global memory in operand shape; there is no LDS.
//
// What differs between the kernels' callers is how a local row becomes a token — a geometry:
//   SidedRows: queries and keys have a buffer, a row stride and a length each; a unit = (sequence, query block).  A packed QKV buffer is
//              the case q = qkv, k = qkv + d, both strides 3d, both lengths L.
//   DiagRows : L <= 16 on one packed buffer: a unit = one 16-row block holding P = floor(16 / L) whole sequences; pairs of different
//              sequences are masked off and have no place in the output.  The last block may be partial: rows are clamped to n_tokens.
// A geometry answers, for a local row of its unit: whether there is such a row, its token, the token to read in place of an absent row
// (the side's spare: such rows are masked / never stored), the sequence within the unit and the position inside it, the
// sequence a query's output row lies in, and which key blocks a causal unit needs.  "Is there such a row" is a 32-bit
// compare of its own, not a -1 among the 64-bit tokens: a sentinel keeps a 64-bit select per key alive through the table below and costs
// a wave of occupancy at three key blocks.  A geometry is built from any kernel-argument struct with the fields Lq, Lk, nqb, P, n_tokens.
#pragma once
#include "common.h"
#include "wave_dpp.h"

struct SidedRows {
  int64_t seq;
  int qb, Lq, Lk;  // qb = the unit's query block
  template <class Geo>
  __device__ __forceinline__ SidedRows(const Geo& g, int64_t unit) : seq(unit / g.nqb), qb((int)(unit - seq * g.nqb)), Lq(g.Lq), Lk(g.Lk) {}
  __device__ __forceinline__ bool q_has(int local) const { return local < Lq; }
  __device__ __forceinline__ bool k_has(int local) const { return local < Lk; }
  __device__ __forceinline__ int64_t q_token(int local) const { return seq * Lq + local; }
  __device__ __forceinline__ int64_t k_token(int local) const { return seq * Lk + local; }
  __device__ __forceinline__ int64_t q_spare() const { return seq * Lq + Lq - 1; }
  __device__ __forceinline__ int64_t k_spare() const { return seq * Lk + Lk - 1; }
  __device__ __forceinline__ int seq_of(int) const { return 0; }  // a unit lies in one sequence
  __device__ __forceinline__ int pos(int local, int) const { return local; }
  __device__ __forceinline__ int64_t out_seq(int) const { return seq; }
  __device__ __forceinline__ bool used(int kb, bool causal) const { return !causal || kb <= qb; }  // causal: Lq == Lk
};

struct DiagRows {
  static constexpr int qb = 0;
  int64_t item, t0, spare;  // the block, its first token, and its last token that exists (taken once: a partial last block clamps it)
  int L, P, rows, n_tokens;
  template <class Geo>
  __device__ __forceinline__ DiagRows(const Geo& g, int64_t unit) : item(unit), t0(unit * (g.P * g.Lk)), L(g.Lk), P(g.P), rows(g.P * g.Lk), n_tokens(g.n_tokens) {
    spare = t0 + rows - 1 > n_tokens - 1 ? n_tokens - 1 : t0 + rows - 1;
  }
  __device__ __forceinline__ bool q_has(int local) const { return local < rows && t0 + local < n_tokens; }
  __device__ __forceinline__ bool k_has(int local) const { return q_has(local); }
  __device__ __forceinline__ int64_t q_token(int local) const { return t0 + local; }
  __device__ __forceinline__ int64_t k_token(int local) const { return t0 + local; }
  __device__ __forceinline__ int64_t q_spare() const { return spare; }
  __device__ __forceinline__ int64_t k_spare() const { return spare; }
  __device__ __forceinline__ int seq_of(int local) const { return local / L; }  // which sequence of the block
  __device__ __forceinline__ int pos(int local, int seq) const { return local - seq * L; }
  __device__ __forceinline__ int64_t out_seq(int q_seq) const { return item * P + q_seq; }
  __device__ __forceinline__ bool used(int, bool) const { return true; }
};

// the spare-token rule: an absent row reads its side's spare token
template <class Rows>
__device__ __forceinline__ int64_t q_read(const Rows& rows, int local) { return rows.q_has(local) ? rows.q_token(local) : rows.q_spare(); }
template <class Rows>
__device__ __forceinline__ int64_t k_read(const Rows& rows, int local) { return rows.k_has(local) ? rows.k_token(local) : rows.k_spare(); }

// per lane: the query of its column (local row q_local) against the four keys of its rows in every key block
template <int NB>
struct Keys16 {
  int pos[NB][4];   // position of the key in its sequence
  bool col[NB][4];  // the pair (query, key) has a place in the output
  bool ok[NB][4];   // ... and is not masked
  int q_seq, q_pos;  // the query's sequence within the unit and its position in it
  // every row's sequence is taken once, ahead of the conditions that use it: inside them the division would be repeated per key
  template <class Rows>
  __device__ __forceinline__ Keys16(const Rows& rows, int q_local, int lg, const uint8_t* kpm, bool causal)
      : q_seq(rows.seq_of(q_local)), q_pos(rows.pos(q_local, q_seq)) {
    const bool q_there = rows.q_has(q_local);
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k_local = kb * 16 + 4 * lg + r;
        const int k_seq = rows.seq_of(k_local);
        pos[kb][r] = rows.pos(k_local, k_seq);
        col[kb][r] = q_there && rows.k_has(k_local) && k_seq == q_seq;
        const bool padded = kpm[k_read(rows, k_local)] != 0;
        ok[kb][r] = col[kb][r] && !padded && (!causal || pos[kb][r] <= q_pos);
      }
    }
  }
};

// a row's 64 floats as four operand fragments: this lane's columns 4 lg .. 4 lg + 3 of every 16 (row already points at column 4 lg)
__device__ __forceinline__ void load_frag16(f32x4 (&f)[4], const float* row) {
#pragma unroll
  for (int c = 0; c < 4; ++c) f[c] = *reinterpret_cast<const f32x4*>(row + 16 * c);
}

// out[kb][r] = rows 4 lg + r of block kb of a (16 NB x 64) · column li of b (16 x 64)^T, for the key blocks the unit uses; zeros elsewhere
template <int NB, class Rows>
__device__ __forceinline__ void scores16(const Rows& rows, bool causal, const f32x4 (&a)[NB][4], const f32x4 (&b)[4], f32x4 (&out)[NB]) {
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
    out[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rows.used(kb, causal)) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) out[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kb][c][e], b[c][e], out[kb], 0, 0, 0);
    }
  }
}

// exp(x) for x <= 0 as exp2 of x * log2(e), the product carried with its rounding error and log2(e)'s own: t = fl(x * L), r = the rest
// of x * log2(e), exp(x) = exp2(t) * (1 + r ln 2).  The plain __expf rounds the product to fp32 — an absolute error of up to ulp(t) / 2
// in the exponent, a relative error of exp of |x| * u: 22 u at x = -40, which is the row's largest element of a gradient-weighted map
// whose peak key has a negative gradient (profiles/explain_scale.md).  This form stays within 2 u (v_exp_f32: 1 ulp); x below -87
// gives 0, as a masked score does — x is clamped at -128 first (exp2(-184) is 0 already), so that a spread near FLT_MAX cannot turn
// t into -inf and 0 * inf into NaN.
__device__ __forceinline__ float exp_nonpos(float x) {
  constexpr float L = 1.44269502162933349609375f, L_REST = 1.92596299e-8f, LN2 = 0.693147182f;
  x = fmaxf(x, -128.f);
  const float t = x * L;
  const float r = fmaf(x, L, -t) + x * L_REST;
  return __builtin_amdgcn_exp2f(t) * fmaf(r, LN2, 1.0f);
}

// mask + softmax of a query's scores (4 per key block, over the 4 lanes lg = 0..3): st becomes exp(score - max), 0 where masked; returns
// 1 / sum, 0 for a row whose keys are all masked (-> zeros).  Domain: a masked score is -1e30 and a score above -1e29 counts as visible,
// so visible scores must lie above -1e29 (those of any fp32 q, k of sane magnitude do).
template <int NB>
__device__ __forceinline__ float softmax16(f32x4 (&st)[NB], const bool (&ok)[NB][4], float scale) {
  float m = -1e30f;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      st[kb][r] = ok[kb][r] ? st[kb][r] * scale : -1e30f;
      m = fmaxf(m, st[kb][r]);
    }
  m = groups_max(m);
  float sum = 0.f;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = st[kb][r] > -1e29f ? exp_nonpos(st[kb][r] - m) : 0.f;
      st[kb][r] = p;
      sum += p;
    }
  sum = groups_sum(sum);
  return sum > 0.f ? 1.0f / sum : 0.f;
}

// this lane's values of one output row; four-byte stores (a row of 7 or 33 floats is not 16-byte aligned)
template <int NB>
__device__ __forceinline__ void store_row16(float* dst, const f32x4 (&p)[NB], const Keys16<NB>& keys) {
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (keys.col[kb][r]) dst[keys.pos[kb][r]] = p[kb][r];
}
