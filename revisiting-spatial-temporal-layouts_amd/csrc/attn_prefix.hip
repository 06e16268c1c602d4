// Probe attention of the per-prefix forward (include/stlt_hip.h: stlt_attn_prefix_probe_fwd, stlt_forward_prefixes).
//
// The temporal tower is causal (reference models.py:136-152), so the logits after t observed frames need, per temporal layer, only one
// more row than the ordinary forward computes: the clip's extract frame placed at position t ("probe" (b,t)), which attends to the frame
// stream's keys j < t and to its own key.  This kernel is that attention for all B*T probes of a layer:
//
//   ctx[b,t,h,:] = softmax( { q_p[b,t]·k_f[b,j]/sqrt(dh) : j < t, kpm[b,j] == 0 }  U  { q_p[b,t]·k_p[b,t]/sqrt(dh) } ) · ( v_f[b,j] ..., v_p[b,t] )
//
// It is memory-bound (it reads the packed rows of both streams once and does T/2 dot products of dh per probe and head), so it runs on the
// vector ALU.  One workgroup of 4 waves owns 32 consecutive probes of one (clip, head); a wave owns 8 of them and keeps their softmax
// state (running maximum, denominator, output row with lane = channel) in registers.  The frame stream's K / V rows are staged in LDS in
// tiles of KT keys, once per workgroup, and every K / V value read from LDS serves the wave's 8 probes; tiles are folded in with the
// online-softmax rescale, so T is not bounded by LDS.  The state starts from the probe's own key (maximum = own score, denominator 1,
// output = v_p): it is always present, the running maximum is finite from the start and masked keys are plain -inf scores.
//   scores : lane = key of the tile, the probes' query rows broadcast from LDS (K rows padded to dh + 4 floats: 16-byte reads that do
//            not collide; head dims that are no multiple of 4 take four-byte reads on rows of an odd pitch)
//   values : lane = channel (dh <= 64 * NC), the probabilities broadcast with v_readlane
#include <cmath>
#include <cstdint>
#include "common.h"
#include "wave_dpp.h"

namespace {

constexpr int PP_WAVES = 4;                   // waves per workgroup
constexpr int PP_QW = 8;                      // probes per wave
constexpr int PP_QB = PP_WAVES * PP_QW;       // probes per workgroup
constexpr int PP_MAX_DH = 256;
constexpr size_t PP_LDS_BYTES = 64 * 1024;    // per workgroup: at head dim 64 a tile of 64 keys + the 32 query rows take 41.5 KiB, 3 workgroups of a CU's 160 KiB

struct ProbeArgs {
  const float* qkv_f; const float* qkv_p; const uint8_t* kpm; float* ctx;
  int T, H, dh, KT, stride, nqb;  // KT: keys per tile; stride: floats per K row in LDS; nqb: workgroups per (clip, head)
  float scale;
};

// rows [0, n_rows) of `src` (row pitch ld, dh floats each) -> LDS rows of pitch `pitch`
template <bool VEC>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int64_t ld, int n_rows, int dh, float* dst, int pitch, int tid) {
  if (VEC) {
    const int dv = dh >> 2;
    for (int i = tid; i < n_rows * dv; i += 64 * PP_WAVES) {
      const int r = i / dv, c = (i - r * dv) * 4;
      *reinterpret_cast<f32x4*>(dst + r * pitch + c) = *reinterpret_cast<const f32x4*>(src + r * ld + c);
    }
  } else {
    for (int i = tid; i < n_rows * dh; i += 64 * PP_WAVES) {
      const int r = i / dh, c = i - r * dh;
      dst[r * pitch + c] = src[r * ld + c];
    }
  }
}

template <int NC, bool VEC>
__global__ __launch_bounds__(64 * PP_WAVES) void attn_prefix_probe_kernel(const ProbeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, H = a.H, dh = a.dh, KT = a.KT, stride = a.stride;
  float* Ks = pp_lds;              // KT rows of `stride` floats
  float* Vs = Ks + KT * stride;    // KT rows of dh floats
  float* Qs = Vs + KT * dh;        // PP_QB rows of dh floats
  float* Ms = Qs + PP_QB * dh;     // KT key flags: 1 = masked
  const int head = (int)(blockIdx.x % (unsigned)H);
  const int64_t rest = blockIdx.x / (unsigned)H;
  const int qb = (int)(rest % a.nqb);
  const int64_t clip = rest / a.nqb;
  const int64_t d = (int64_t)H * dh, ld = 3 * d, hoff = (int64_t)head * dh;
  const int t_blk = qb * PP_QB;                               // first probe of the workgroup
  const int n_q = T - t_blk < PP_QB ? T - t_blk : PP_QB;      // its probes (>= 1)
  const float* __restrict__ p_rows = a.qkv_p + (clip * T + t_blk) * ld + hoff;  // probe rows: q at +0, k at +d, v at +2d
  const float* __restrict__ f_rows = a.qkv_f + clip * T * ld + hoff;
  stage_rows<VEC>(p_rows, ld, n_q, dh, Qs, dh, tid);
  __syncthreads();

  const int r0 = wave * PP_QW;      // the wave's first probe inside the workgroup's block
  const bool active = r0 < n_q;
  int rq[PP_QW];                    // LDS query row of probe qi (probes past the clip's end repeat the last one; nothing of them is stored)
  float m[PP_QW], l[PP_QW], acc[PP_QW][NC];
#pragma unroll
  for (int qi = 0; qi < PP_QW; ++qi) {
    rq[qi] = r0 + qi < n_q ? r0 + qi : n_q - 1;
    const float* __restrict__ prow = p_rows + rq[qi] * ld;
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      acc[qi][i] = 0.f;
      if (c < dh) {
        part += Qs[rq[qi] * dh + c] * prow[d + c];
        acc[qi][i] = prow[2 * d + c];
      }
    }
    m[qi] = wave_sum_dpp(part) * a.scale;  // the own key opens the softmax: maximum = its score, denominator 1, output = v_p
    l[qi] = 1.f;
  }

  const int t_wmax = t_blk + (r0 + PP_QW < n_q ? r0 + PP_QW : n_q) - 1;  // the wave's last probe: it sees keys j < t_wmax
  const int n_keys = t_blk + n_q - 1;                                   // keys the workgroup's last probe sees
  for (int j0 = 0; j0 < n_keys; j0 += KT) {
    const int nk = n_keys - j0 < KT ? n_keys - j0 : KT;
    __syncthreads();  // the previous tile is read
    stage_rows<VEC>(f_rows + j0 * ld + d, ld, nk, dh, Ks, stride, tid);
    stage_rows<VEC>(f_rows + j0 * ld + 2 * d, ld, nk, dh, Vs, dh, tid);
    for (int i = tid; i < nk; i += 64 * PP_WAVES) Ms[i] = a.kpm[clip * T + j0 + i] ? 1.f : 0.f;
    __syncthreads();
    if (!active || j0 >= t_wmax) continue;  // wave-uniform
    const int nkw = t_wmax - j0 < nk ? t_wmax - j0 : nk;
    const int kl = lane < nk ? lane : nk - 1;  // lanes past the tile's keys repeat its last one (their scores are masked)
    const float* krow = Ks + kl * stride;
    float sc[PP_QW];
#pragma unroll
    for (int qi = 0; qi < PP_QW; ++qi) sc[qi] = 0.f;
    if (VEC) {
      for (int c = 0; c < dh; c += 4) {
        const f32x4 kv = *reinterpret_cast<const f32x4*>(krow + c);
#pragma unroll
        for (int qi = 0; qi < PP_QW; ++qi) {
          const f32x4 qv = *reinterpret_cast<const f32x4*>(Qs + rq[qi] * dh + c);
          sc[qi] += kv[0] * qv[0] + kv[1] * qv[1] + kv[2] * qv[2] + kv[3] * qv[3];
        }
      }
    } else {
      for (int c = 0; c < dh; ++c) {
        const float kv = krow[c];
#pragma unroll
        for (int qi = 0; qi < PP_QW; ++qi) sc[qi] += kv * Qs[rq[qi] * dh + c];
      }
    }
    const bool key_ok = lane < nk && Ms[kl] == 0.f;
    const int j = j0 + lane;
    float p[PP_QW];
#pragma unroll
    for (int qi = 0; qi < PP_QW; ++qi) {
      const int t = t_blk + r0 + qi;
      const float sv = (key_ok && j < t) ? sc[qi] * a.scale : -INFINITY;
      const float mn = fmaxf(m[qi], wave_max_dpp(sv));  // finite: m is
      const float alpha = expf(m[qi] - mn);
      p[qi] = expf(sv - mn);
      l[qi] = l[qi] * alpha + wave_sum_dpp(p[qi]);
      m[qi] = mn;
#pragma unroll
      for (int i = 0; i < NC; ++i) acc[qi][i] *= alpha;
    }
    for (int jj = 0; jj < nkw; ++jj) {
      float pj[PP_QW];
#pragma unroll
      for (int qi = 0; qi < PP_QW; ++qi)
        pj[qi] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, p[qi]), jj));
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (c < dh) {
          const float v = Vs[jj * dh + c];
#pragma unroll
          for (int qi = 0; qi < PP_QW; ++qi) acc[qi][i] = fmaf(pj[qi], v, acc[qi][i]);
        }
      }
    }
  }

#pragma unroll
  for (int qi = 0; qi < PP_QW; ++qi) {
    if (r0 + qi < n_q) {
      float* __restrict__ out = a.ctx + (clip * T + t_blk + r0 + qi) * d + hoff;
      const float inv = 1.0f / l[qi];
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (c < dh) out[c] = acc[qi][i] * inv;
      }
    }
  }
}

__global__ __launch_bounds__(256) void prefix_zero_invalid_kernel(float* __restrict__ logits, const int64_t* __restrict__ lengths, int64_t n, int T, int K) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int64_t row = idx / K;  // b * T + t
  const int64_t b = row / T;
  if (row - b * T >= lengths[b]) logits[idx] = 0.f;
}

template <int NC>
void launch_probe_nc(bool vec, dim3 grid, size_t lds, hipStream_t s, const ProbeArgs& a) {
  if (vec) hipLaunchKernelGGL((attn_prefix_probe_kernel<NC, true>), grid, dim3(64 * PP_WAVES), lds, s, a);
  else hipLaunchKernelGGL((attn_prefix_probe_kernel<NC, false>), grid, dim3(64 * PP_WAVES), lds, s, a);
}

}  // namespace

int launch_attn_prefix_probe(const float* qkv_frames, const float* qkv_probes, const uint8_t* kpm, int64_t S, int64_t T, int64_t H, int64_t dh,
                             float* ctx, hipStream_t s) {
  if (!qkv_frames || !qkv_probes || !kpm || !ctx) return stlt_set_error(STLT_EINVAL, "stlt_attn_prefix_probe_fwd: null pointer");
  if (dh < 1 || dh > PP_MAX_DH) return stlt_set_error(STLT_EINVAL, "stlt_attn_prefix_probe_fwd: head dim %lld unsupported (1 ... %d)", (long long)dh, PP_MAX_DH);
  if (S < 0 || T <= 0 || H <= 0 || H > 65535 || T > 0x7fffff00LL) return stlt_set_error(STLT_EINVAL, "stlt_attn_prefix_probe_fwd: bad clip / frame / head count");
  if (const char* off = stlt_first_unaligned16({{"qkv_frames", qkv_frames}, {"qkv_probes", qkv_probes}, {"ctx", ctx}}))
    return stlt_set_error(STLT_EINVAL, "stlt_attn_prefix_probe_fwd: %s must be 16-byte aligned", off);
  if (S == 0) return 0;
  const int64_t nqb = (T + PP_QB - 1) / PP_QB;
  if (S * nqb * H > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_attn_prefix_probe_fwd: too many (clip, head) items");
  const bool vec = dh % 4 == 0;  // with 16-byte bases, every q / k / v slice of a packed row then starts on 16 bytes
  const int stride = vec ? (int)dh + 4 : ((int)dh | 1);
  // the largest tile of 64 / 32 / 16 / 8 keys that fits beside the query rows (head dim 256: 8 keys)
  const size_t fixed = (size_t)PP_QB * dh * sizeof(float);
  const size_t per_key = ((size_t)stride + dh + 1) * sizeof(float);
  int KT = 64;
  while (KT > 8 && fixed + KT * per_key > PP_LDS_BYTES) KT >>= 1;
  const size_t lds = fixed + KT * per_key;
  if (lds > PP_LDS_BYTES) return stlt_set_error(STLT_EINVAL, "stlt_attn_prefix_probe_fwd: head dim %lld does not fit the LDS budget", (long long)dh);
  ProbeArgs a{qkv_frames, qkv_probes, kpm, ctx, (int)T, (int)H, (int)dh, KT, stride, (int)nqb, 1.0f / sqrtf((float)dh)};
  StltProfScope ps(STLT_K_ATTN_TEMPORAL, s);
  stlt_prof_note("attn_prefix_probe S=%lld T=%lld H=%lld dh=%lld KT=%d", (long long)S, (long long)T, (long long)H, (long long)dh, KT);
  stlt_prof_add_bytes((double)S * T * H * dh * 4.0 * (2 + 3 + 1) + (double)S * T);  // frame K/V, probe q/k/v, ctx, mask
  stlt_prof_note_flops((double)S * H * T * (T + 1) * 2.0 * dh);                    // (T-1)/2 + 1 keys per probe on average, two dot products each
  const dim3 grid((unsigned)(S * nqb * H));
  if (dh <= 64) launch_probe_nc<1>(vec, grid, lds, s, a);
  else if (dh <= 128) launch_probe_nc<2>(vec, grid, lds, s, a);
  else launch_probe_nc<4>(vec, grid, lds, s, a);
  return stlt_check_launch("attn_prefix_probe_kernel");
}

int launch_prefix_zero_invalid(float* logits, const int64_t* lengths, int64_t B, int64_t T, int64_t K, hipStream_t s) {
  if (!logits || !lengths) return stlt_set_error(STLT_EINVAL, "stlt_forward_prefixes: null logits / lengths");
  const int64_t n = B * T * K;
  if (n <= 0) return 0;
  if ((n + 255) / 256 > 0x7fffffffLL) return stlt_set_error(STLT_EINVAL, "stlt_forward_prefixes: too many logits");
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("prefix_zero_invalid rows=%lld K=%lld", (long long)(B * T), (long long)K);
  hipLaunchKernelGGL(prefix_zero_invalid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, logits, lengths, n, (int)T, (int)K);
  return stlt_check_launch("prefix_zero_invalid_kernel");
}
