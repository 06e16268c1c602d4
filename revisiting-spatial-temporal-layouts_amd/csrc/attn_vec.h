// Small device helpers of the vector-ALU attention kernels (attn_any.hip, the generic paths of attn_probs.hip and attn_grad_probs.hip): one wave per query row,
// the query broadcast from LDS.  The wave-wide sum beside wave_max is common.h's wave_sum.
#pragma once
#include "common.h"

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  return x;
}
// LDS traffic of one wave is in order; this keeps the compiler from moving accesses across and drains the counters
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// dot product of a row in LDS with a row in global memory (VEC: both 16-byte aligned, n % 4 == 0)
template <bool VEC>
__device__ __forceinline__ float dot_row(const float* __restrict__ s, const float* __restrict__ g, int n) {
  float acc = 0.f;
  if (VEC) {
    for (int c = 0; c < n; c += 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(s + c);
      const f32x4 b = *reinterpret_cast<const f32x4*>(g + c);
      acc += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    }
  } else {
    for (int c = 0; c < n; ++c) acc += s[c] * g[c];
  }
  return acc;
}
