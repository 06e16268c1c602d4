// Integrated gradients (Sundararajan, Taly, Yan 2017) on the device: the attribution of one logit to every input element is
// (x - x0) * the integral of d logit / d x along the straight path from a baseline x0 to the input x, by the trapezoid rule on
// S = steps + 1 points.  The expensive part — a tape forward and an input-only reverse sweep per path point — exists (train.hip, r3d.hip);
// this file is what makes the rest cheap: the interpolated batches of a pass in one launch, the quadrature in a fixed order, and the
// completeness gap sum(attr) - seed . (F(x) - F(x0)) reduced on the device.
//
//   ig_path_kernel        a layout batch at steps s0 .. s1, step-major: boxes and scores interpolated, every other tensor moved as the
//                         integer it is stored as.  One thread per object slot reads the slot once and writes every step from registers.
//   ig_path_dense_kernel  one dense float32 tensor (video_frames, appearance_features) at steps s0 .. s1: 16-byte accesses on the aligned
//                         body, a scalar head and tail (VEC); one float per access when the pointers' alignments disagree.
//   ig_reduce_kernel      acc <- acc + w_s * g_s for s ascending, one element per lane; the finishing call multiplies by (x - x0) and,
//                         when asked, sums groups of consecutive attributions (the four box coordinates of a slot, plus its score term).
//   ig_delta_*_kernel     stage 1: one fp32 partial per chunk of IG_DELTA_CHUNK attributions (a fixed partition: the chunk, not the grid,
//                         decides who adds what); stage 2: one workgroup per clip adds the partials and the logit term in fp64.
//
// The arithmetic (include/stlt_hip.h spells it out): alpha_s = s / steps and the weights are IEEE fp32 quotients; the path point is
// fadd(x0, fmul(alpha_s, fsub(x, x0))), the accumulation fadd(acc, fmul(w_s, g_s)) — separately rounded, never contracted into an FMA
// (the pragma below; build.py passes -ffp-contract=off for this file as well), so a numpy float32 restatement gives the same bits.
#include <cstring>
#include "common.h"
#include "wave_dpp.h"

#pragma clang fp contract(off)

namespace {

constexpr int IG_THREADS = 256;
constexpr int IG_MAX_STEPS = STLT_IG_MAX_STEPS;
constexpr int IG_DELTA_CHUNK = STLT_IG_DELTA_CHUNK;  // attributions of one stage-1 partial
constexpr int IG_GRID = 256 * 8;                     // grid-stride launches: eight workgroups for each of the chip's 256 CUs

// The quotient of two integers below 2^24 in fp32, correctly rounded: the fp64 quotient rounded once more is the fp32 quotient whenever
// the wider format has at least 2 * 24 + 2 digits (Figueroa 1995), so this does not depend on how a float division is expanded.
__device__ __forceinline__ float ig_quot(int a, int b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float ig_alpha(int s, int steps) { return ig_quot(s, steps); }
__device__ __forceinline__ float ig_weight(int s, int steps) { return (s == 0 || s == steps) ? ig_quot(1, 2 * steps) : ig_quot(1, steps); }
// step 0 is the baseline's bits and step `steps` the input's: neither is computed
__device__ __forceinline__ float ig_point(float x, float x0, int s, int steps) {
  if (s == 0) return x0;
  if (s == steps) return x;
  return __fadd_rn(x0, __fmul_rn(ig_alpha(s, steps), __fsub_rn(x, x0)));
}

struct IgBatch {  // the tensors of a collated batch (scores may be null), in or out
  int64_t* categories; float* boxes; float* scores; uint8_t* kpm_boxes; int64_t* frame_types; uint8_t* kpm_frames; int64_t* lengths;
};

// One workgroup per (clip, IG_THREADS object slots); the clip's first workgroup also moves the frame tensors and the length.
__global__ __launch_bounds__(IG_THREADS) void ig_path_kernel(IgBatch in, const float* __restrict__ boxes0, const float* __restrict__ scores0, int64_t B, int T, int N,
                                                             int parts, int steps, int s0, int n_steps, IgBatch out) {
  const int64_t b = blockIdx.x / parts;
  const int part = (int)(blockIdx.x - b * parts);
  const int tid = threadIdx.x;
  const int64_t slots = (int64_t)T * N;
  const int64_t i = (int64_t)part * IG_THREADS + tid;
  if (i < slots) {
    const int64_t src = b * slots + i;
    const int64_t cat = in.categories[src];
    const uint8_t m = in.kpm_boxes[src];
    float x[4], x0[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = in.boxes[src * 4 + c];
    if (boxes0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) x0[c] = boxes0[src * 4 + c];
    }
    const float sc = in.scores ? in.scores[src] : 0.f;
    const float sc0 = (in.scores && scores0) ? scores0[src] : 0.f;
    for (int ds = 0; ds < n_steps; ++ds) {
      const int s = s0 + ds;
      const int64_t dst = ((int64_t)ds * B + b) * slots + i;
      out.categories[dst] = cat;
      out.kpm_boxes[dst] = m;
#pragma unroll
      for (int c = 0; c < 4; ++c) out.boxes[dst * 4 + c] = ig_point(x[c], x0[c], s, steps);
      if (in.scores) out.scores[dst] = ig_point(sc, sc0, s, steps);
    }
  }
  if (part == 0) {
    for (int t = tid; t < T; t += IG_THREADS) {
      const int64_t ft = in.frame_types[b * T + t];
      const uint8_t mf = in.kpm_frames[b * T + t];
      for (int ds = 0; ds < n_steps; ++ds) {
        const int64_t dst = ((int64_t)ds * B + b) * T + t;
        out.frame_types[dst] = ft;
        out.kpm_frames[dst] = mf;
      }
    }
    if (tid == 0) {
      const int64_t len = in.lengths[b];
      for (int ds = 0; ds < n_steps; ++ds) out.lengths[(int64_t)ds * B + b] = len;
    }
  }
}

// x, x0 and out are flat: `total` = B * n elements, step ds of the output at out + ds * total.  VEC: elements [head, head + 4 * vecs) are
// moved as float4 (the launcher made sure that x + head, x0 + head and every out + ds * total + head are 16-byte aligned); the at most
// three elements before and after them go one by one through the first lanes of workgroup 0.
template <bool VEC>
__global__ __launch_bounds__(IG_THREADS) void ig_path_dense_kernel(const float* __restrict__ x, const float* __restrict__ x0, float fill, int64_t total, int head,
                                                                   int64_t vecs, int steps, int s0, int n_steps, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * IG_THREADS;
  const int64_t first = (int64_t)blockIdx.x * IG_THREADS + threadIdx.x;
  if constexpr (VEC) {
    for (int64_t v = first; v < vecs; v += stride) {
      const int64_t e = head + 4 * v;
      const float4 a = *reinterpret_cast<const float4*>(x + e);
      const float4 a0 = x0 ? *reinterpret_cast<const float4*>(x0 + e) : make_float4(fill, fill, fill, fill);
      for (int ds = 0; ds < n_steps; ++ds) {
        const int s = s0 + ds;
        float4 p;
        p.x = ig_point(a.x, a0.x, s, steps);
        p.y = ig_point(a.y, a0.y, s, steps);
        p.z = ig_point(a.z, a0.z, s, steps);
        p.w = ig_point(a.w, a0.w, s, steps);
        *reinterpret_cast<float4*>(out + (int64_t)ds * total + e) = p;
      }
    }
    if (blockIdx.x == 0) {
      const int64_t tail0 = head + 4 * vecs;  // lanes [0, head) take the head, lanes [head, head + tail) the tail: at most six in all
      const int64_t e = threadIdx.x < head ? (int64_t)threadIdx.x : tail0 + (threadIdx.x - head);
      if (e < total) {
        const float a = x[e], a0 = x0 ? x0[e] : fill;
        for (int ds = 0; ds < n_steps; ++ds) out[(int64_t)ds * total + e] = ig_point(a, a0, s0 + ds, steps);
      }
    }
  } else {
    for (int64_t e = first; e < total; e += stride) {
      const float a = x[e], a0 = x0 ? x0[e] : fill;
      for (int ds = 0; ds < n_steps; ++ds) out[(int64_t)ds * total + e] = ig_point(a, a0, s0 + ds, steps);
    }
  }
}

// One lane per group of `group` consecutive elements (group == 1 unless the call sums groups).  acc is read unless `begin`, the steps are
// added in ascending s, acc is written back; `finish` multiplies by (x - x0) and adds the group's attributions left to right, then extra.
__global__ __launch_bounds__(IG_THREADS) void ig_reduce_kernel(const float* __restrict__ g, int64_t total, int group, int steps, int s0, int n_steps, int begin, int finish,
                                                               float* __restrict__ acc, const float* __restrict__ x, const float* __restrict__ x0, float fill,
                                                               float* __restrict__ attr, const float* __restrict__ extra, float* __restrict__ grouped) {
  const int64_t stride = (int64_t)gridDim.x * IG_THREADS;
  const int64_t groups = total / group;
  for (int64_t j = (int64_t)blockIdx.x * IG_THREADS + threadIdx.x; j < groups; j += stride) {
    float sum = 0.f;
    for (int c = 0; c < group; ++c) {
      const int64_t e = j * group + c;
      float a = begin ? 0.f : acc[e];
      for (int ds = 0; ds < n_steps; ++ds) a = __fadd_rn(a, __fmul_rn(ig_weight(s0 + ds, steps), g[(int64_t)ds * total + e]));
      acc[e] = a;
      if (finish) {
        const float v = __fmul_rn(__fsub_rn(x[e], x0 ? x0[e] : fill), a);
        attr[e] = v;
        sum = c == 0 ? v : __fadd_rn(sum, v);
      }
    }
    if (finish && grouped) grouped[j] = extra ? __fadd_rn(sum, extra[j]) : sum;
  }
}

struct IgDeltaParts {  // up to three attribution tensors of n[i] elements per clip; tensor i owns chunks [first[i], first[i+1]) of a clip's `chunks`
  const float* a[3];
  int64_t n[3];
  int first[4];
};

// Stage 1.  Chunk q of clip b: lane t adds elements t, t + 256, ... of the chunk in that order, the wave adds its lanes on the DPP path,
// the four waves are added pairwise.  The workgroups stride over the B * chunks chunks, so the grid changes who computes a partial, never how.
__global__ __launch_bounds__(IG_THREADS) void ig_delta_partial_kernel(IgDeltaParts p, int64_t B, int chunks, float* __restrict__ partial) {
  __shared__ float wave_part[IG_THREADS / 64];
  const int64_t all = B * chunks;
  for (int64_t q = blockIdx.x; q < all; q += gridDim.x) {
    const int64_t b = q / chunks;
    const int c = (int)(q - b * chunks);
    const int i = c >= p.first[2] ? 2 : (c >= p.first[1] ? 1 : 0);
    const int64_t lo = (int64_t)(c - p.first[i]) * IG_DELTA_CHUNK;
    const int64_t hi = lo + IG_DELTA_CHUNK < p.n[i] ? lo + IG_DELTA_CHUNK : p.n[i];
    const float* a = p.a[i] + b * p.n[i];
    float s = 0.f;
    for (int64_t e = lo + threadIdx.x; e < hi; e += IG_THREADS) s += a[e];
    s = wave_sum_dpp(s);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[q] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
    __syncthreads();
  }
}

__device__ __forceinline__ double ig_block_sum(double v, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();
  return r;
}

// Stage 2.  One workgroup per clip: the clip's partials and the K products seed * (logits_x - logits_x0), each summed in fp64 in a fixed
// order, one rounding to fp32 at the end.
__global__ __launch_bounds__(IG_THREADS) void ig_delta_final_kernel(const float* __restrict__ partial, int chunks, const float* __restrict__ seed,
                                                                    const float* __restrict__ lx, const float* __restrict__ lx0, int K, float* __restrict__ delta) {
  __shared__ double lds[IG_THREADS / 64];
  const int64_t b = blockIdx.x;
  double s = 0.0;
  for (int c = threadIdx.x; c < chunks; c += IG_THREADS) s += (double)partial[b * chunks + c];
  const double attr = ig_block_sum(s, lds);
  double t = 0.0;
  for (int k = threadIdx.x; k < K; k += IG_THREADS) t += (double)seed[b * K + k] * ((double)lx[b * K + k] - (double)lx0[b * K + k]);
  const double gap = ig_block_sum(t, lds);
  if (threadIdx.x == 0) delta[b] = (float)(attr - gap);
}

// the shared step check -> an error message, or null
const char* ig_steps(int64_t steps, int64_t s0, int64_t s1) {
  if (steps < 1 || steps >= (1 << 23)) return "steps must be in [1, 2^23)";
  if (s0 < 0 || s0 > s1 || s1 > steps) return "0 <= s0 <= s1 <= steps";
  if (s1 - s0 + 1 > IG_MAX_STEPS) return "more than 256 steps in one call (split the range)";
  return nullptr;
}

unsigned ig_grid(int64_t items) {
  const int64_t blocks = (items + IG_THREADS - 1) / IG_THREADS;
  return (unsigned)(blocks < 1 ? 1 : (blocks < IG_GRID ? blocks : IG_GRID));
}

const char* ig_delta_layout(int64_t B, const int64_t n[3], int64_t* chunks, int first[4]) {
  if (B < 0 || B > 0x7fffffff) return "bad batch size";
  int64_t c = 0;
  for (int i = 0; i < 3; ++i) {
    if (n[i] < 0 || n[i] >= (1ll << 31)) return "a tensor holds 2^31 elements per clip or more (or fewer than 0)";
    first[i] = (int)c;
    c += (n[i] + IG_DELTA_CHUNK - 1) / IG_DELTA_CHUNK;
  }
  first[3] = (int)c;
  if (c < 1) return "no attribution tensor";
  if (B > 0 && c > (int64_t)0x7fffffff / B) return "2^31 chunks or more";
  *chunks = c;
  return nullptr;
}

}  // namespace

extern "C" {

int stlt_ig_path(const stlt_inputs* in, const float* boxes0, const float* scores0, int64_t steps, int64_t s0, int64_t s1, int64_t* categories, float* boxes,
                 float* scores, uint8_t* kpm_boxes, int64_t* frame_types, uint8_t* kpm_frames, int64_t* lengths, stlt_stream_t stream) {
  if (!in) return stlt_set_error(STLT_EINVAL, "stlt_ig_path: null pointer");
  const int64_t B = in->B, T = in->T, N = in->N;
  if (B < 0 || T <= 0 || N <= 0 || T > 0x7fffffff || N > 0x7fffffff || B > 0x7fffffff || T > (0x7fffffff / 4) / N || (B > 0 && T * N * 4 > 0x7fffffff / B))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_path: bad shape (B=%lld, T=%lld, N=%lld): boxes hold fewer than 2^31 elements", (long long)B, (long long)T, (long long)N);
  if (const char* why = ig_steps(steps, s0, s1))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_path: %s (got steps=%lld, s0=%lld, s1=%lld)", why, (long long)steps, (long long)s0, (long long)s1);
  if (B == 0) return 0;
  if (!in->categories || !in->boxes || !in->kpm_boxes || !in->frame_types || !in->kpm_frames || !in->lengths || !categories || !boxes || !kpm_boxes || !frame_types ||
      !kpm_frames || !lengths || (in->scores && !scores))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_path: null pointer");
  const int64_t parts = (T * N + IG_THREADS - 1) / IG_THREADS;
  if (parts > 0x7fffffff / B) return stlt_set_error(STLT_EINVAL, "stlt_ig_path: %lld workgroups in one call (at most 2^31 - 1)", (long long)(parts * B));
  IgBatch src{const_cast<int64_t*>(in->categories), const_cast<float*>(in->boxes), const_cast<float*>(in->scores), const_cast<uint8_t*>(in->kpm_boxes),
              const_cast<int64_t*>(in->frame_types), const_cast<uint8_t*>(in->kpm_frames), const_cast<int64_t*>(in->lengths)};
  IgBatch dst{categories, boxes, in->scores ? scores : nullptr, kpm_boxes, frame_types, kpm_frames, lengths};
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("ig_path B=%lld T=%lld N=%lld steps=%lld [%lld,%lld]", (long long)B, (long long)T, (long long)N, (long long)steps, (long long)s0, (long long)s1);
  hipLaunchKernelGGL(ig_path_kernel, dim3((unsigned)(parts * B)), dim3(IG_THREADS), 0, s, src, boxes0, scores0, B, (int)T, (int)N, (int)parts, (int)steps, (int)s0,
                     (int)(s1 - s0 + 1), dst);
  return stlt_check_launch("ig_path_kernel");
}

int stlt_ig_path_dense(const float* x, const float* x0, float fill, int64_t B, int64_t n, int64_t steps, int64_t s0, int64_t s1, float* out, stlt_stream_t stream) {
  if (B < 0 || n <= 0 || B > 0x7fffffff || n > 0x7fffffff || (B > 0 && n > 0x7fffffff / B))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_path_dense: bad shape (B=%lld, n=%lld): the tensor holds fewer than 2^31 elements", (long long)B, (long long)n);
  if (const char* why = ig_steps(steps, s0, s1))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_path_dense: %s (got steps=%lld, s0=%lld, s1=%lld)", why, (long long)steps, (long long)s0, (long long)s1);
  if (B == 0) return 0;
  if (!x || !out) return stlt_set_error(STLT_EINVAL, "stlt_ig_path_dense: null pointer");
  const int64_t total = B * n, n_steps = s1 - s0 + 1;
  const uintptr_t ax = reinterpret_cast<uintptr_t>(x) & 15, a0 = reinterpret_cast<uintptr_t>(x0) & 15, ao = reinterpret_cast<uintptr_t>(out) & 15;
  // one misalignment for all three pointers (a multiple of 4 bytes), and every step of the output as misaligned as the first
  const bool vec = (ax & 3) == 0 && ao == ax && (!x0 || a0 == ax) && (n_steps == 1 || total % 4 == 0);
  const int head = vec ? (int)(((16 - ax) & 15) / 4) : 0;
  const int64_t vecs = vec && total > head ? (total - head) / 4 : 0;
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("ig_path_dense B=%lld n=%lld steps=%lld [%lld,%lld] vec=%d head=%d", (long long)B, (long long)n, (long long)steps, (long long)s0, (long long)s1, (int)vec, head);
  if (vec)
    hipLaunchKernelGGL(ig_path_dense_kernel<true>, dim3(ig_grid(vecs)), dim3(IG_THREADS), 0, s, x, x0, fill, total, head, vecs, (int)steps, (int)s0, (int)n_steps, out);
  else
    hipLaunchKernelGGL(ig_path_dense_kernel<false>, dim3(ig_grid(total)), dim3(IG_THREADS), 0, s, x, x0, fill, total, 0, (int64_t)0, (int)steps, (int)s0, (int)n_steps, out);
  return stlt_check_launch("ig_path_dense_kernel");
}

int stlt_ig_reduce(const float* g, int64_t B, int64_t n, int64_t steps, int64_t s0, int64_t s1, int flags, float* acc, const float* x, const float* x0, float fill,
                   float* attr, int64_t group, const float* extra, float* grouped, stlt_stream_t stream) {
  if (B < 0 || n <= 0 || B > 0x7fffffff || n > 0x7fffffff || (B > 0 && n > 0x7fffffff / B))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_reduce: bad shape (B=%lld, n=%lld): the tensor holds fewer than 2^31 elements", (long long)B, (long long)n);
  if (const char* why = ig_steps(steps, s0, s1))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_reduce: %s (got steps=%lld, s0=%lld, s1=%lld)", why, (long long)steps, (long long)s0, (long long)s1);
  if (flags & ~(STLT_IG_BEGIN | STLT_IG_FINISH)) return stlt_set_error(STLT_EINVAL, "stlt_ig_reduce: flags are STLT_IG_BEGIN | STLT_IG_FINISH, got %d", flags);
  const bool finish = (flags & STLT_IG_FINISH) != 0;
  if (grouped ? (!finish || group < 1 || group > 64 || n % group != 0) : (group > 1 || extra != nullptr))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_reduce: grouped takes STLT_IG_FINISH and 1 <= group <= 64 dividing n; group and extra need grouped (group=%lld, n=%lld)",
                          (long long)group, (long long)n);
  if (B == 0) return 0;
  if (!g || !acc || (finish && (!x || !attr))) return stlt_set_error(STLT_EINVAL, "stlt_ig_reduce: null pointer (x and attr are required with STLT_IG_FINISH)");
  const int64_t total = B * n;
  const int grp = grouped ? (int)group : 1;
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("ig_reduce B=%lld n=%lld steps=%lld [%lld,%lld] flags=%d group=%d", (long long)B, (long long)n, (long long)steps, (long long)s0, (long long)s1, flags, grp);
  hipLaunchKernelGGL(ig_reduce_kernel, dim3(ig_grid(total / grp)), dim3(IG_THREADS), 0, s, g, total, grp, (int)steps, (int)s0, (int)(s1 - s0 + 1),
                     (flags & STLT_IG_BEGIN) ? 1 : 0, finish ? 1 : 0, acc, x, x0, fill, attr, extra, grouped);
  return stlt_check_launch("ig_reduce_kernel");
}

size_t stlt_ig_delta_scratch_bytes(int64_t B, int64_t n0, int64_t n1, int64_t n2) {
  const int64_t n[3] = {n0, n1, n2};
  int64_t chunks;
  int first[4];
  if (ig_delta_layout(B, n, &chunks, first)) return 0;
  return (size_t)B * (size_t)chunks * sizeof(float);
}

int stlt_ig_delta(const float* a0, int64_t n0, const float* a1, int64_t n1, const float* a2, int64_t n2, const float* seed, const float* logits_x,
                  const float* logits_x0, int64_t B, int64_t K, int64_t max_blocks, void* scratch, size_t scratch_bytes, float* delta, stlt_stream_t stream) {
  IgDeltaParts p{{a0, a1, a2}, {n0, n1, n2}, {0, 0, 0, 0}};
  int64_t chunks;
  if (const char* why = ig_delta_layout(B, p.n, &chunks, p.first))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_delta: %s (B=%lld, n=(%lld,%lld,%lld))", why, (long long)B, (long long)n0, (long long)n1, (long long)n2);
  if (K <= 0 || K > 0x7fffffff || (B > 0 && K > 0x7fffffff / B)) return stlt_set_error(STLT_EINVAL, "stlt_ig_delta: bad shape (B=%lld, K=%lld)", (long long)B, (long long)K);
  if (max_blocks < 0 || max_blocks > 0x7fffffff) return stlt_set_error(STLT_EINVAL, "stlt_ig_delta: max_blocks is 0 (the default) or a grid size, got %lld", (long long)max_blocks);
  if (B == 0) return 0;
  if ((n0 > 0 && !a0) || (n1 > 0 && !a1) || (n2 > 0 && !a2) || !seed || !logits_x || !logits_x0 || !scratch || !delta)
    return stlt_set_error(STLT_EINVAL, "stlt_ig_delta: null pointer");
  const size_t need = (size_t)B * (size_t)chunks * sizeof(float);
  if (scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 3))
    return stlt_set_error(STLT_EINVAL, "stlt_ig_delta: scratch holds %zu bytes, needs %zu (stlt_ig_delta_scratch_bytes), 4-byte aligned", scratch_bytes, need);
  const int64_t all = B * chunks, cap = max_blocks > 0 ? max_blocks : IG_GRID;
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("ig_delta B=%lld n=(%lld,%lld,%lld) K=%lld chunks=%lld", (long long)B, (long long)n0, (long long)n1, (long long)n2, (long long)K, (long long)chunks);
  float* partial = static_cast<float*>(scratch);
  hipLaunchKernelGGL(ig_delta_partial_kernel, dim3((unsigned)(all < cap ? all : cap)), dim3(IG_THREADS), 0, s, p, B, (int)chunks, partial);
  if (int rc = stlt_check_launch("ig_delta_partial_kernel")) return rc;
  hipLaunchKernelGGL(ig_delta_final_kernel, dim3((unsigned)B), dim3(IG_THREADS), 0, s, partial, (int)chunks, seed, logits_x, logits_x0, (int)K, delta);
  return stlt_check_launch("ig_delta_final_kernel");
}

}  // extern "C"
