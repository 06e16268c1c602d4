// R3D-50 video trunk (reference src/modelling/resnets3d.py:93-214, generate_model(50) minus avgpool / fc; models.py:198-228).
// Activations are channels-last (NDHWC) inside the trunk, so every Conv3d is an implicit GEMM
//   y (M = B·To·Ho·Wo, N = Cout) = x_taps (M, K = kt·kh·kw·Cin) · wᵀ,   w repacked to (Cout, kt, kh, kw, Cin)
// on v_mfma_f32_16x16x4_f32 with fp32 accumulation, the reference's own arithmetic.  Epilogue: eval BatchNorm
// (γ·(v - mean)/sqrt(var + eps) + β from the BN buffers), an optional residual of the output's shape, then ReLU.
//
// The activation operand is gathered with ordinary bounds-checked 16-byte loads into registers and written to LDS, not by LDS-DMA:
// a padding tap (and a row past M, a k past K) must read as zero, which a DMA cannot mask, and pointing padded rows at a zeroed device
// row would still need a per-lane address select plus a zero buffer the caller has to provide.  The register stage also overlaps the
// next k-slab's loads with the current slab's MFMAs.  Channel counts must be multiples of 4 (a 16-byte quad never straddles two taps);
// the stem's Cin = 3 is padded to 4 by the input-layout kernel and the repack, so one (dt, dh) row of its taps is 28 contiguous floats.
//
// Launches with fewer output tiles than the chip has room for (layer 4 at small batches: M = 128 rows for 4 clips) split the
// contraction: split z writes its raw partial tile to a slab of the workspace, and a second launch sums the slabs in split order and
// applies the epilogue — deterministic, no atomics.  The split plan is host arithmetic over the shape alone (not the device), so a given
// shape always runs the same summation order.
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include "common.h"

namespace {

constexpr int CK = 32;         // k-slab width (floats)
constexpr int LDS_PITCH = CK + 4;
constexpr int BM = 128;        // output rows per workgroup
constexpr int64_t SPLIT_TARGET_WG = 512;   // split under-filled launches up to ~2 workgroups per CU of a 256-CU part
constexpr int64_t SPLIT_MIN_SLABS = 8;     // ... but keep at least 8 k-slabs (256 of K) per split
constexpr int64_t SPLIT_MAX = 64;

struct ConvGeom {
  int B, Ti, Hi, Wi, C;        // input NDHWC, C = channels as stored (multiple of 4)
  int To, Ho, Wo, N;           // output NDHWC (N = Cout)
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
  int M, K;                    // M = B·To·Ho·Wo, K = kt·kh·kw·C
};

__device__ __forceinline__ void bn_coeffs(const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var, float eps, int n,
                                          float* sc, float* sh) {
  if (bn_w) {
    const float s = bn_w[n] / sqrtf(bn_var[n] + eps);
    *sc = s;
    *sh = bn_b[n] - bn_mean[n] * s;
  } else {
    *sc = 1.f;
    *sh = 0.f;
  }
}

// One workgroup: a BM x BN output tile, 4 waves of (BM/2) x (BN/2), each a grid of 16 x 16 MFMA blocks.  LDS holds both operand tiles
// row-major ([row][k], pitch 36 floats).  The 32 k of a slab are visited in the order k = 8·lg + s (lane group lg, step s = 0..7), the
// same for both operands, so a lane fetches its eight k of a row with two 16-byte LDS reads.  Staging: eight lanes cover one row's
// 128-byte slab (coalesced), a thread keeps BM/32 (BN/32) fixed rows and one fixed k-quad.
// gridDim.z > 1: blockIdx.z takes k-slabs [z·per, (z+1)·per) and stores the raw partial to y + z·M·N (no epilogue).
// Backward epilogue (BWD = true, the data gradient of csrc/r3d.hip's stlt_conv3d_bwd_data): output row gm of the (compact) launch
// grid lands at row dest(gm) of the full dx grid (Tf, Hf, Wf): position os·(t, h, w) + (ot, oh, ow), so one parity class of a
// stride-2 convolution writes only its own rows.  v = acc · sc[n] (sc NULL: 1), + add[row] (NULL: none), then 0 unless mask[row] > 0
// (NULL: no mask).  `add` may be dx itself (each element is read and then written by the same thread).
struct DgEpi {
  const float* sc;
  const float* mask;
  const float* add;
  int Tf, Hf, Wf, os, ot, oh, ow;
};

__device__ __forceinline__ int64_t dg_row(const ConvGeom& g, const DgEpi& e, int gm) {
  int q = gm;
  const int wo = q % g.Wo; q /= g.Wo;
  const int ho = q % g.Ho; q /= g.Ho;
  const int to = q % g.To; const int b = q / g.To;
  return (((int64_t)b * e.Tf + e.os * to + e.ot) * e.Hf + e.os * ho + e.oh) * e.Wf + e.os * wo + e.ow;
}

__device__ __forceinline__ float dg_apply(const DgEpi& e, float v, int n, int64_t o) {
  if (e.sc) v *= e.sc[n];
  if (e.add) v += e.add[o];
  if (e.mask && !(e.mask[o] > 0.f)) v = 0.f;
  return v;
}

template <int BN, bool BWD = false>
__global__ __launch_bounds__(256) void conv3d_igemm_kernel(const float* __restrict__ x, const float* __restrict__ w, ConvGeom g,
                                                           const float* __restrict__ bn_w, const float* __restrict__ bn_b,
                                                           const float* __restrict__ bn_mean, const float* __restrict__ bn_var, float eps,
                                                           const float* __restrict__ res, int relu, float* y, int slabs_per_split, DgEpi de) {
  constexpr int RA = BM / 32, RB = BN / 32, MI = BM / 32, NJ = BN / 32;
  __shared__ __attribute__((aligned(16))) float As[BM][LDS_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[BN][LDS_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int srow = tid >> 3, kq = (tid & 7) * 4;

  // the thread's staged activation rows: batch offset and the window origin (t0, h0, w0); rows past M never pass the bounds test
  int64_t xb[RA];
  int t0[RA], h0[RA], w0[RA];
#pragma unroll
  for (int e = 0; e < RA; ++e) {
    const int m = m0 + srow + 32 * e;
    if (m < g.M) {
      int q = m;
      const int wo = q % g.Wo; q /= g.Wo;
      const int ho = q % g.Ho; q /= g.Ho;
      const int to = q % g.To; const int b = q / g.To;
      xb[e] = (int64_t)b * g.Ti * g.Hi * g.Wi * g.C;
      t0[e] = to * g.st - g.pt; h0[e] = ho * g.sh - g.ph; w0[e] = wo * g.sw - g.pw;
    } else {
      xb[e] = 0; t0[e] = -(1 << 28); h0[e] = 0; w0[e] = 0;
    }
  }

  const int n_slabs = (g.K + CK - 1) / CK;
  int s_begin = 0, s_end = n_slabs;
  if (gridDim.z > 1) {
    s_begin = blockIdx.z * slabs_per_split;
    s_end = min(n_slabs, s_begin + slabs_per_split);
    y += (int64_t)blockIdx.z * g.M * g.N;
  }

  f32x4 ra[RA], rb[RB];
  auto load_slab = [&](int slab) {
    const int k = slab * CK + kq;
    const bool kin = k < g.K;
    int dt = 0, dh = 0, dw = 0, c = 0;
    if (kin) {
      int tap = k / g.C;
      c = k - tap * g.C;
      dw = tap % g.kw; tap /= g.kw;
      dh = tap % g.kh; dt = tap / g.kh;
    }
#pragma unroll
    for (int e = 0; e < RA; ++e) {
      const int ti = t0[e] + dt, hi = h0[e] + dh, wi = w0[e] + dw;
      if (kin && (unsigned)ti < (unsigned)g.Ti && (unsigned)hi < (unsigned)g.Hi && (unsigned)wi < (unsigned)g.Wi)
        ra[e] = *reinterpret_cast<const f32x4*>(x + xb[e] + (((int64_t)ti * g.Hi + hi) * g.Wi + wi) * g.C + c);
      else
        ra[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int e = 0; e < RB; ++e) {
      const int n = n0 + srow + 32 * e;
      rb[e] = (kin && n < g.N) ? *reinterpret_cast<const f32x4*>(w + (int64_t)n * g.K + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (s_begin < s_end) load_slab(s_begin);
  for (int slab = s_begin; slab < s_end; ++slab) {
#pragma unroll
    for (int e = 0; e < RA; ++e) *reinterpret_cast<f32x4*>(&As[srow + 32 * e][kq]) = ra[e];
#pragma unroll
    for (int e = 0; e < RB; ++e) *reinterpret_cast<f32x4*>(&Bs[srow + 32 * e][kq]) = rb[e];
    __syncthreads();
    if (slab + 1 < s_end) load_slab(slab + 1);  // in flight during this slab's MFMAs
    f32x4 a[MI][2], b[NJ][2];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      a[i][0] = *reinterpret_cast<const f32x4*>(&As[wm + 16 * i + li][8 * lg]);
      a[i][1] = *reinterpret_cast<const f32x4*>(&As[wm + 16 * i + li][8 * lg + 4]);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      b[j][0] = *reinterpret_cast<const f32x4*>(&Bs[wn + 16 * j + li][8 * lg]);
      b[j][1] = *reinterpret_cast<const f32x4*>(&Bs[wn + 16 * j + li][8 * lg + 4]);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s >> 2][s & 3], b[j][s >> 2][s & 3], acc[i][j], 0, 0, 0);
    __syncthreads();
  }

  const bool split = gridDim.z > 1;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int gn = n0 + wn + 16 * j + li;
    if (gn >= g.N) continue;
    float sc = 1.f, sh = 0.f;
    if (!BWD && !split) bn_coeffs(bn_w, bn_b, bn_mean, bn_var, eps, gn, &sc, &sh);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int gm = m0 + wm + 16 * i + 4 * lg + q;
        if (gm >= g.M) continue;
        const int64_t o = (int64_t)gm * g.N + gn;
        if (split) { y[o] = acc[i][j][q]; continue; }
        if constexpr (BWD) {
          const int64_t od = dg_row(g, de, gm) * g.N + gn;
          y[od] = dg_apply(de, acc[i][j][q], gn, od);
          continue;
        }
        float v = fmaf(acc[i][j][q], sc, sh);
        if (res) v += res[o];
        if (relu) v = fmaxf(v, 0.f);
        y[o] = v;
      }
  }
}

// the split launch's second half: y = epilogue(part[0] + part[1] + ...), slabs summed in split order
__global__ __launch_bounds__(256) void conv3d_split_finish_kernel(const float* __restrict__ part, int splits, int M, int N, const float* __restrict__ bn_w,
                                                                  const float* __restrict__ bn_b, const float* __restrict__ bn_mean,
                                                                  const float* __restrict__ bn_var, float eps, const float* __restrict__ res, int relu,
                                                                  float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)M * N;
  if (idx >= total) return;
  const int n = (int)(idx % N);
  float v = 0.f;
  for (int z = 0; z < splits; ++z) v += part[(int64_t)z * total + idx];
  float sc, sh;
  bn_coeffs(bn_w, bn_b, bn_mean, bn_var, eps, n, &sc, &sh);
  v = fmaf(v, sc, sh);
  if (res) v += res[idx];
  if (relu) v = fmaxf(v, 0.f);
  y[idx] = v;
}

// (Cout, Cin, kt, kh, kw) -> (Cout, kt, kh, kw, Cpad), channels Cin .. Cpad-1 zero
__global__ __launch_bounds__(256) void conv3d_repack_kernel(const float* __restrict__ w, int64_t Cout, int Cin, int taps, int Cpad, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Cout * taps * Cpad) return;
  const int c = (int)(idx % Cpad);
  const int64_t r = idx / Cpad;
  const int tap = (int)(r % taps);
  const int64_t n = r / taps;
  out[idx] = c < Cin ? w[(n * Cin + c) * taps + tap] : 0.f;
}

// NCDHW (B, C, T, H, W) -> NDHWC (B, T, H, W, Cpad), channels C .. Cpad-1 zero
__global__ __launch_bounds__(256) void ncdhw_to_ndhwc_kernel(const float* __restrict__ x, int64_t B, int C, int64_t P, int Cpad, float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * P * Cpad) return;
  const int c = (int)(idx % Cpad);
  const int64_t r = idx / Cpad;
  const int64_t p = r % P, b = r / P;
  y[idx] = c < C ? x[(b * C + c) * P + p] : 0.f;
}

// NDHWC (B, P, C) -> NCDHW (B, C, P)
__global__ __launch_bounds__(256) void ndhwc_to_ncdhw_kernel(const float* __restrict__ x, int64_t B, int64_t P, int C, float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * P * C) return;
  const int64_t p = idx % P;
  const int64_t r = idx / P;
  const int c = (int)(r % C);
  const int64_t b = r / C;
  y[idx] = x[(b * P + p) * C + c];
}

// MaxPool3d(kernel 3, stride 2, padding 1) in NDHWC (resnets3d.py:124): padding taps are -inf, i.e. skipped
__global__ __launch_bounds__(256) void maxpool3d_ndhwc_kernel(const float* __restrict__ x, int B, int T, int H, int W, int C, int To, int Ho, int Wo,
                                                              float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * To * Ho * Wo * C) return;
  const int c = (int)(idx % C);
  int64_t q = idx / C;
  const int wo = (int)(q % Wo); q /= Wo;
  const int ho = (int)(q % Ho); q /= Ho;
  const int to = (int)(q % To);
  const int64_t b = q / To;
  float m = -INFINITY;
  for (int dt = 0; dt < 3; ++dt) {
    const int t = 2 * to - 1 + dt;
    if ((unsigned)t >= (unsigned)T) continue;
    for (int dh = 0; dh < 3; ++dh) {
      const int h = 2 * ho - 1 + dh;
      if ((unsigned)h >= (unsigned)H) continue;
      for (int dw = 0; dw < 3; ++dw) {
        const int ww = 2 * wo - 1 + dw;
        if ((unsigned)ww >= (unsigned)W) continue;
        m = fmaxf(m, x[(((b * T + t) * H + h) * W + ww) * C + c]);
      }
    }
  }
  y[idx] = m;
}

// global average pool of NDHWC (B, P, C) -> (B, C): positions summed in order, then divided by P
__global__ __launch_bounds__(256) void avgpool_ndhwc_kernel(const float* __restrict__ x, int64_t B, int P, int C, float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * C) return;
  const int c = (int)(idx % C);
  const int64_t b = idx / C;
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += x[(b * P + p) * C + c];
  y[idx] = s / (float)P;
}

inline int64_t out_dim(int64_t in, int64_t k, int64_t s, int64_t p) { return (in + 2 * p - k) / s + 1; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int conv_bn_tile(int64_t N) { return N <= 64 ? 64 : 128; }

// Π v > limit for non-negative factors, without forming a product past the limit: the shape checks bound each extent by 2^24 (or not
// at all: a batch), so a product of four or five of them overflows int64 before any limit could be applied to it
inline bool prod_over(std::initializer_list<int64_t> v, int64_t limit) {
  int64_t p = 1;
  for (int64_t x : v) {
    if (x > 0 && p > limit / x) return true;
    p *= x;
  }
  return false;
}

// The split arithmetic of every launcher and workspace query, forward (k-slabs), data gradient (k-slabs of a parity class) and weight
// gradient (m-slabs): a request of `want` ranges over `slabs` slabs becomes at most one range per slab, every range cdiv(slabs, ranges)
// slabs long (the last may be shorter), so the count can come out below the request.  No slabs, or want <= 1: one range.
struct SplitRanges { int64_t splits, per; };
inline SplitRanges split_ranges(int64_t slabs, int64_t want) {
  if (slabs <= 0 || want <= 1) return {1, slabs > 0 ? slabs : 1};
  const int64_t per = cdiv(slabs, std::min(want, slabs));
  return {cdiv(slabs, per), per};
}

// number of contraction splits for an (M, N, K) conv launch (1: whole tiles, no workspace)
int64_t conv_plan_splits(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = cdiv(M, BM) * cdiv(N, conv_bn_tile(N));
  const int64_t slabs = cdiv(K, CK);
  if (tiles >= SPLIT_TARGET_WG / 2) return 1;
  int64_t splits = cdiv(SPLIT_TARGET_WG, tiles);
  if (splits > slabs / SPLIT_MIN_SLABS) splits = slabs / SPLIT_MIN_SLABS;
  if (splits > SPLIT_MAX) splits = SPLIT_MAX;
  return split_ranges(slabs, splits).splits;
}

int check_desc(const stlt_conv3d_desc* d, ConvGeom* g) {
  if (!d) return stlt_set_error(STLT_EINVAL, "conv3d: null descriptor");
  const int64_t v[] = {d->B, d->T, d->H, d->W, d->c_in, d->c_out, d->kt, d->kh, d->kw, d->st, d->sh, d->sw};
  for (int64_t x : v)
    if (x <= 0 || x > (1 << 24)) return stlt_set_error(STLT_EINVAL, "conv3d: sizes, kernel and stride must be positive");
  if (d->pt < 0 || d->ph < 0 || d->pw < 0 || d->pt >= d->kt || d->ph >= d->kh || d->pw >= d->kw)
    return stlt_set_error(STLT_EINVAL, "conv3d: padding must lie in [0, kernel)");
  if (d->c_in % 4) return stlt_set_error(STLT_EINVAL, "conv3d: c_in must be a multiple of 4 (pad the channels: stlt_ncdhw_to_ndhwc, stlt_conv3d_repack), got %lld", (long long)d->c_in);
  const int64_t To = out_dim(d->T, d->kt, d->st, d->pt), Ho = out_dim(d->H, d->kh, d->sh, d->ph), Wo = out_dim(d->W, d->kw, d->sw, d->pw);
  if (To <= 0 || Ho <= 0 || Wo <= 0) return stlt_set_error(STLT_EINVAL, "conv3d: the kernel is larger than the padded input");
  if (prod_over({d->B, To, Ho, Wo}, 0x7fffff00LL) || prod_over({d->kt, d->kh, d->kw, d->c_in}, 0x7fffff00LL) ||
      prod_over({d->B, d->T, d->H, d->W}, 0x7fffff00LL) || prod_over({d->B, To, Ho, Wo, d->c_out}, 1LL << 40))
    return stlt_set_error(STLT_EINVAL, "conv3d: shape too large");
  const int64_t M = d->B * To * Ho * Wo, K = d->kt * d->kh * d->kw * d->c_in;
  if (cdiv(M, BM) > 0x7fffffffLL || cdiv(d->c_out, 64) > 65535) return stlt_set_error(STLT_EINVAL, "conv3d: too many output tiles");
  *g = ConvGeom{(int)d->B, (int)d->T, (int)d->H, (int)d->W, (int)d->c_in, (int)To, (int)Ho, (int)Wo, (int)d->c_out, (int)d->kt, (int)d->kh, (int)d->kw,
                (int)d->st, (int)d->sh, (int)d->sw, (int)d->pt, (int)d->ph, (int)d->pw, (int)M, (int)K};
  return 0;
}

int64_t conv_split_bytes(const ConvGeom& g, int64_t splits) { return splits > 1 ? splits * (int64_t)g.M * g.N * (int64_t)sizeof(float) : 0; }

// the forward's split count for a caller's n_split (<= 0: the plan for the shape)
int64_t conv_splits(const ConvGeom& g, int n_split) { return n_split <= 0 ? conv_plan_splits(g.M, g.N, g.K) : split_ranges(cdiv(g.K, CK), n_split).splits; }

int launch_conv(const ConvGeom& g, const float* x, const float* w, const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var,
                float eps, const float* res, int relu, float* y, int64_t want_splits, float* part, hipStream_t s) {
  const int bn = conv_bn_tile(g.N);
  const auto [splits, per] = split_ranges(cdiv(g.K, CK), want_splits);
  const dim3 grid((unsigned)cdiv(g.M, BM), (unsigned)cdiv(g.N, bn), (unsigned)splits), block(256);
  float* dst = splits > 1 ? part : y;
  const DgEpi none{};
  if (bn == 64)
    hipLaunchKernelGGL(conv3d_igemm_kernel<64>, grid, block, 0, s, x, w, g, bn_w, bn_b, bn_mean, bn_var, eps, res, relu, dst, (int)per, none);
  else
    hipLaunchKernelGGL(conv3d_igemm_kernel<128>, grid, block, 0, s, x, w, g, bn_w, bn_b, bn_mean, bn_var, eps, res, relu, dst, (int)per, none);
  if (int e = stlt_check_launch("conv3d_igemm_kernel")) return e;
  if (splits > 1) {
    hipLaunchKernelGGL(conv3d_split_finish_kernel, dim3((unsigned)cdiv((int64_t)g.M * g.N, 256)), dim3(256), 0, s, part, (int)splits, g.M, g.N, bn_w, bn_b,
                       bn_mean, bn_var, eps, res, relu, y);
    return stlt_check_launch("conv3d_split_finish_kernel");
  }
  return 0;
}

// the shape check of the three max-pool entry points
int check_pool_shape(const char* who, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C) {
  if (B < 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || T > (1 << 24) || H > (1 << 24) || W > (1 << 24) || C > (1 << 24) || prod_over({B, T, H, W, C}, 1LL << 40))
    return stlt_set_error(STLT_EINVAL, "%s: bad shape", who);
  return 0;
}

}  // namespace

extern "C" {

size_t stlt_conv3d_workspace_bytes(const stlt_conv3d_desc* d, int n_split) {
  ConvGeom g;
  if (check_desc(d, &g)) return 0;
  return (size_t)conv_split_bytes(g, conv_splits(g, n_split));
}

int stlt_conv3d_fwd(const stlt_conv3d_desc* d, const float* x, const float* w, const float* bn_w, const float* bn_b, const float* bn_mean,
                    const float* bn_var, float bn_eps, const float* residual, int relu, int n_split, void* workspace, size_t workspace_bytes, float* y,
                    stlt_stream_t stream) {
  ConvGeom g;
  if (int e = check_desc(d, &g)) return e;
  if (!x || !w || !y) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_fwd: null pointer");
  if (bn_w && (!bn_b || !bn_mean || !bn_var)) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_fwd: BatchNorm needs all four of weight, bias, running mean, running var");
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15)) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_fwd: x and w must be 16-byte aligned");
  if (n_split < 0 || n_split > 1024) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_fwd: n_split must lie in [0, 1024]");
  int64_t splits = conv_splits(g, n_split);
  if (n_split == 0 && (!workspace || workspace_bytes < (size_t)conv_split_bytes(g, splits))) splits = 1;  // automatic: split only into lent workspace
  if (splits > 1 && (!workspace || workspace_bytes < (size_t)conv_split_bytes(g, splits)))
    return stlt_set_error(STLT_EWORKSPACE, "stlt_conv3d_fwd: %lld splits need %lld workspace bytes, %zu lent", (long long)splits,
                          (long long)conv_split_bytes(g, splits), workspace_bytes);
  return launch_conv(g, x, w, bn_w, bn_b, bn_mean, bn_var, bn_eps, residual, relu, y, splits, (float*)workspace, (hipStream_t)stream);
}

int stlt_conv3d_repack(const float* w, int64_t c_out, int64_t c_in, int64_t kt, int64_t kh, int64_t kw, int64_t c_pad, float* out, stlt_stream_t stream) {
  if (!w || !out) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_repack: null pointer");
  if (c_out <= 0 || c_in <= 0 || kt <= 0 || kh <= 0 || kw <= 0 || c_pad < c_in || c_pad > (1 << 20) || prod_over({kt, kh, kw}, 1 << 20) || c_out > (1 << 24) ||
      prod_over({c_out, kt, kh, kw, c_pad}, 1LL << 40))
    return stlt_set_error(STLT_EINVAL, "stlt_conv3d_repack: bad shape");
  const int64_t n = c_out * kt * kh * kw * c_pad;
  hipLaunchKernelGGL(conv3d_repack_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w, c_out, (int)c_in, (int)(kt * kh * kw),
                     (int)c_pad, out);
  return stlt_check_launch("conv3d_repack_kernel");
}

int stlt_ncdhw_to_ndhwc(const float* x, int64_t B, int64_t C, int64_t T, int64_t H, int64_t W, int64_t c_pad, float* y, stlt_stream_t stream) {
  if (!x || !y) return stlt_set_error(STLT_EINVAL, "stlt_ncdhw_to_ndhwc: null pointer");
  if (B < 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || c_pad < C || c_pad > (1 << 20) || prod_over({B, T, H, W, c_pad}, 1LL << 40))
    return stlt_set_error(STLT_EINVAL, "stlt_ncdhw_to_ndhwc: bad shape");
  const int64_t n = B * T * H * W * c_pad;
  if (n == 0) return 0;
  hipLaunchKernelGGL(ncdhw_to_ndhwc_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, B, (int)C, T * H * W, (int)c_pad, y);
  return stlt_check_launch("ncdhw_to_ndhwc_kernel");
}

int stlt_ndhwc_to_ncdhw(const float* x, int64_t B, int64_t P, int64_t C, float* y, stlt_stream_t stream) {
  if (!x || !y) return stlt_set_error(STLT_EINVAL, "stlt_ndhwc_to_ncdhw: null pointer");
  if (B < 0 || P <= 0 || C <= 0 || C > (1 << 24) || prod_over({B, P, C}, 1LL << 40)) return stlt_set_error(STLT_EINVAL, "stlt_ndhwc_to_ncdhw: bad shape");
  const int64_t n = B * P * C;
  if (n == 0) return 0;
  hipLaunchKernelGGL(ndhwc_to_ncdhw_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, B, P, (int)C, y);
  return stlt_check_launch("ndhwc_to_ncdhw_kernel");
}

int stlt_maxpool3d_ndhwc(const float* x, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, float* y, stlt_stream_t stream) {
  if (!x || !y) return stlt_set_error(STLT_EINVAL, "stlt_maxpool3d_ndhwc: null pointer");
  if (int e = check_pool_shape("stlt_maxpool3d_ndhwc", B, T, H, W, C)) return e;
  const int64_t To = out_dim(T, 3, 2, 1), Ho = out_dim(H, 3, 2, 1), Wo = out_dim(W, 3, 2, 1);
  const int64_t n = B * To * Ho * Wo * C;
  if (n == 0) return 0;
  hipLaunchKernelGGL(maxpool3d_ndhwc_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, (int)B, (int)T, (int)H, (int)W, (int)C,
                     (int)To, (int)Ho, (int)Wo, y);
  return stlt_check_launch("maxpool3d_ndhwc_kernel");
}

int stlt_avgpool_ndhwc(const float* x, int64_t B, int64_t P, int64_t C, float* y, stlt_stream_t stream) {
  if (!x || !y) return stlt_set_error(STLT_EINVAL, "stlt_avgpool_ndhwc: null pointer");
  if (B < 0 || P <= 0 || C <= 0 || P > (1 << 24) || C > (1 << 24) || prod_over({B, P, C}, 1LL << 40)) return stlt_set_error(STLT_EINVAL, "stlt_avgpool_ndhwc: bad shape");
  if (B == 0) return 0;
  hipLaunchKernelGGL(avgpool_ndhwc_kernel, dim3((unsigned)cdiv(B * C, 256)), dim3(256), 0, (hipStream_t)stream, x, B, (int)P, (int)C, y);
  return stlt_check_launch("avgpool_ndhwc_kernel");
}

}  // extern "C"

// =====================================================================================================================================
// Backward (training the trunk).  BatchNorm is always eval (frozen affine, running statistics), so the backward of bn(conv(x)) is
// a per-channel multiply by sc = γ/sqrt(var + eps); ReLU masks by its saved output > 0.
//
// Data gradient (dgrad): dx = the forward kernel (conv3d_igemm_kernel<BN, true>) run over dy with a repacked weight
//   W'[ci][taps'][co] = sc[co] · W[co][ci][flipped taps]
// and the backward epilogue (scale, add-source, mask, scattered rows: DgEpi).  A stride-s dimension splits into s parity classes
// r (input positions s·a + r): class r takes exactly the taps dt with (r + p - dt) ≡ 0 mod s, as a dense stride-1 convolution over dy
// with k' = their count and padding p' (sub_dims).  Stride 1 is the single class with the full flipped kernel and p' = k - 1 - p;
// a 3x3x3 stride-2 conv becomes 8 classes of 1 or 2 taps per dimension (27 taps in all, none of them zero); a 1x1x1 stride-2 conv
// has one class with its tap and seven with none (those rows get only the add-source, masked).  The classes' weights lie back to
// back in class order (rt, rh, rw row-major), so the dgrad copy has as many floats as the weight.
//
// Weight gradient (wgrad): dW[co][tap, c] = Σ_m dy[m][co] · x_taps[m][tap, c] over M = B·To·Ho·Wo.  Both operands are M-major with
// channels contiguous; a thread stages one m row (one decode per slab) and fixed channel quads, written transposed into LDS
// ([co or k][m], pitch 36) so the MFMA loop is the forward's.  M splits into ranges whose partial (c_out, K) slabs are summed in split
// order by a finishing pass, which applies sc[co], drops padded channels, writes the torch layout (c_out, c_in, kt, kh, kw) and
// optionally accumulates into it — deterministic, no float atomics.
// =====================================================================================================================================
namespace {

constexpr int WG_TK = 128;                 // wgrad tile: k columns per workgroup (co rows: 64 or 128)
constexpr int64_t WG_TARGET_WG = 1024;     // split M until ~4 workgroups per CU of a 256-CU part
constexpr int64_t WG_MIN_SLABS = 8;        // ... keeping at least 8 m-slabs (256 rows) per split
constexpr int64_t WG_SPLIT_MAX = 256;

// the taps of parity class r of one dimension (kernel k, stride s, pad p): k' taps (0: none), padding p' of the stride-1 sub-conv
__host__ __device__ inline void sub_dims(int k, int s, int p, int r, int* kk, int* pp) {
  int qmin = 1 << 30, qmax = -(1 << 30);
  for (int dt = 0; dt < k; ++dt) {
    const int num = r + p - dt;
    if (((num % s) + s) % s) continue;
    const int q = (num >= 0) ? num / s : -((-num) / s);
    qmin = q < qmin ? q : qmin;
    qmax = q > qmax ? q : qmax;
  }
  *kk = qmax >= qmin ? qmax - qmin + 1 : 0;
  *pp = qmax >= qmin ? -qmin : 0;
}

// (c_out, c_in, kt, kh, kw) -> the dgrad copy (classes back to back, each (c_in, kt', kh', kw', c_out)), scaled by sc[co]
// (sc from `scale`, or from BatchNorm weight / running var, or 1)
// (I: the index type — int inside the trunk's batched repack, int64_t for an arbitrary op-level shape)
template <typename I>
__device__ inline void dgrad_repack_elem(const float* w, I idx, int Cout, int Cin, int kt, int kh, int kw, int st, int sh, int sw, int pt, int ph,
                                         int pw, float sc, float* out) {
  // idx walks the source (co, ci, dt, dh, dw)
  I q = idx;
  const int dw = (int)(q % kw); q /= kw;
  const int dh = (int)(q % kh); q /= kh;
  const int dt = (int)(q % kt); q /= kt;
  const int ci = (int)(q % Cin);
  const int co = (int)(q / Cin);
  const int rt = ((dt - pt) % st + st) % st, rh = ((dh - ph) % sh + sh) % sh, rw = ((dw - pw) % sw + sw) % sw;
  int64_t base = 0;
  int kt_ = 0, kh_ = 0, kw_ = 0, pt_ = 0, ph_ = 0, pw_ = 0;
  for (int a = 0; a < st; ++a)
    for (int b = 0; b < sh; ++b)
      for (int c = 0; c < sw; ++c) {
        int k1, k2, k3, p1, p2, p3;
        sub_dims(kt, st, pt, a, &k1, &p1);
        sub_dims(kh, sh, ph, b, &k2, &p2);
        sub_dims(kw, sw, pw, c, &k3, &p3);
        if (a == rt && b == rh && c == rw) {
          kt_ = k1; kh_ = k2; kw_ = k3; pt_ = p1; ph_ = p2; pw_ = p3;
          a = st; b = sh; break;
        }
        base += (int64_t)k1 * k2 * k3 * Cin * Cout;
      }
  const int jt = (rt + pt - dt) / st + pt_, jh = (rh + ph - dh) / sh + ph_, jw = (rw + pw - dw) / sw + pw_;
  out[base + ((((int64_t)ci * kt_ + jt) * kh_ + jh) * kw_ + jw) * Cout + co] = sc * w[idx];
}

__global__ __launch_bounds__(256) void conv3d_repack_dgrad_kernel(const float* __restrict__ w, int Cout, int Cin, int kt, int kh, int kw, int st, int sh,
                                                                  int sw, int pt, int ph, int pw, const float* __restrict__ scale, float* __restrict__ out) {
  const int64_t n = (int64_t)Cout * Cin * kt * kh * kw;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
    const int co = (int)(idx / ((int64_t)Cin * kt * kh * kw));
    dgrad_repack_elem(w, idx, Cout, Cin, kt, kh, kw, st, sh, sw, pt, ph, pw, scale ? scale[co] : 1.f, out);
  }
}

// the trunk's fixed plan, conv i in state-dict order: (c_out, c_in, k, stride); the stem is 7x7x7 stride (1, 2, 2) pad 3.
// The one statement of which block has a downsample and which stride: the batched repack reads it on the device, trunk_plan on the host.
struct R3dConvMeta { int cout, cin, k, s; };
__host__ __device__ inline R3dConvMeta r3d_conv_meta(int i) {
  if (i == 0) return {64, 3, 7, 2};
  const int blocks[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512};
  int idx = 1, cin = 64;
  for (int L = 0; L < 4; ++L)
    for (int b = 0; b < blocks[L]; ++b) {
      const int pl = planes[L], s = (L > 0 && b == 0) ? 2 : 1;
      if (i == idx) return {pl, cin, 1, 1};
      if (i == idx + 1) return {pl, pl, 3, s};
      if (i == idx + 2) return {pl * 4, pl, 1, 1};
      if (b == 0 && i == idx + 3) return {pl * 4, cin, 1, s};
      idx += b == 0 ? 4 : 3;
      cin = pl * 4;
    }
  return {0, 0, 0, 0};
}

constexpr int REPACK_ITEMS = 4;  // elements per thread of r3d_repack_all_kernel (1 024 per workgroup)

struct R3dRepackArgs {
  const float* w[STLT_R3D_CONVS];
  const float* bn_w[STLT_R3D_CONVS];
  const float* bn_var[STLT_R3D_CONVS];
  float* fwd[STLT_R3D_CONVS];
  float* dgrad[STLT_R3D_CONVS];
  int block0[STLT_R3D_CONVS + 1];  // conv i owns workgroups [block0[i], block0[i + 1]): one flat index space, sized per conv
  float eps;
};

// conv i's elements in r3d_repack_all_kernel: its forward copy, then (but for the stem) its dgrad copy
__host__ __device__ inline void r3d_repack_counts(int i, int* nf, int* nw) {
  const R3dConvMeta m = r3d_conv_meta(i);
  const int taps = m.k * m.k * m.k;
  *nf = m.cout * taps * ((m.cin + 3) / 4 * 4);
  *nw = i > 0 ? m.cout * m.cin * taps : 0;
}

// one workgroup = 1 024 consecutive elements of one conv: the forward copy (c_out, k, k, k, c_pad), walked in destination order
// (coalesced stores), then the BN-scaled dgrad copy, walked in source order (coalesced loads)
__global__ __launch_bounds__(256) void r3d_repack_all_kernel(R3dRepackArgs a) {
  int i = 0;
  while (i + 1 < STLT_R3D_CONVS && (int)blockIdx.x >= a.block0[i + 1]) ++i;
  const R3dConvMeta m = r3d_conv_meta(i);
  const int taps = m.k * m.k * m.k, cpad = (m.cin + 3) / 4 * 4;
  int nf, nw;
  r3d_repack_counts(i, &nf, &nw);
  const float* w = a.w[i];
  const int base = ((int)blockIdx.x - a.block0[i]) * 256 * REPACK_ITEMS + threadIdx.x;
#pragma unroll
  for (int e = 0; e < REPACK_ITEMS; ++e) {
    const int idx = base + 256 * e;
    if (idx < nf) {
      if (!a.fwd[i]) continue;
      const int c = idx % cpad;
      const int r = idx / cpad;
      const int tap = r % taps;
      const int n = r / taps;
      a.fwd[i][idx] = c < m.cin ? w[((int64_t)n * m.cin + c) * taps + tap] : 0.f;
    } else if (idx - nf < nw && a.dgrad[i]) {
      const int j = idx - nf;
      const int co = j / (m.cin * taps);
      const float sc = a.bn_w[i][co] / sqrtf(a.bn_var[i][co] + a.eps);
      const int pd = m.k / 2;
      dgrad_repack_elem(w, j, m.cout, m.cin, m.k, m.k, m.k, m.s, m.s, m.s, pd, pd, pd, sc, a.dgrad[i]);
    }
  }
}

// split dgrad launch, second half: row gm of the compact grid = Σ_z part[z] (split order), then the backward epilogue at dest(gm)
__global__ __launch_bounds__(256) void conv3d_dgrad_finish_kernel(const float* __restrict__ part, int splits, ConvGeom g, DgEpi de, float* y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)g.M * g.N;
  if (idx >= total) return;
  const int n = (int)(idx % g.N);
  const int gm = (int)(idx / g.N);
  float v = 0.f;
  for (int z = 0; z < splits; ++z) v += part[(int64_t)z * total + idx];
  const int64_t od = dg_row(g, de, gm) * g.N + n;
  y[od] = dg_apply(de, v, n, od);
}

// wgrad main loop: tile TA (co) x WG_TK (k); blockIdx.z = split: m-slabs [z·per, (z+1)·per); raw partial -> part + z·N·K
// (g is the FORWARD geometry: x (B, Ti, Hi, Wi, C), dy (M, N))
template <int TA>
__global__ __launch_bounds__(256) void conv3d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, ConvGeom g, float* __restrict__ part,
                                                           int slabs_per_split) {
  constexpr int TB = WG_TK, RA = TA / 32, RB = TB / 32, MI = TA / 32, NJ = TB / 32;
  __shared__ __attribute__((aligned(16))) float As[TA][LDS_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[TB][LDS_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int wm = (wave >> 1) * (TA / 2), wn = (wave & 1) * (TB / 2);
  const int co0 = blockIdx.x * TA, k0 = blockIdx.y * TB;
  const int mr = tid & 31, cq = tid >> 5;  // this thread's m row within a slab; its channel quads are cq + 8e

  // fixed k-quads of the x operand: tap offsets and channel
  int dt[RB], dh[RB], dw[RB], cc[RB];
  bool kin[RB];
#pragma unroll
  for (int e = 0; e < RB; ++e) {
    const int k = k0 + 4 * (cq + 8 * e);
    kin[e] = k < g.K;
    int tap = kin[e] ? k / g.C : 0;
    cc[e] = kin[e] ? k - tap * g.C : 0;
    dw[e] = tap % g.kw; tap /= g.kw;
    dh[e] = tap % g.kh; dt[e] = tap / g.kh;
  }

  const int n_slabs = (g.M + CK - 1) / CK;
  const int s_begin = blockIdx.z * slabs_per_split, s_end = min(n_slabs, s_begin + slabs_per_split);
  part += (int64_t)blockIdx.z * g.N * g.K;

  f32x4 ra[RA], rb[RB];
  auto load_slab = [&](int slab) {
    const int m = slab * CK + mr;
    const bool min_ = m < g.M;
    int64_t xb = 0;
    int t0 = 0, h0 = 0, w0 = 0;
    if (min_) {
      int q = m;
      const int wo = q % g.Wo; q /= g.Wo;
      const int ho = q % g.Ho; q /= g.Ho;
      const int to = q % g.To; const int b = q / g.To;
      xb = (int64_t)b * g.Ti * g.Hi * g.Wi * g.C;
      t0 = to * g.st - g.pt; h0 = ho * g.sh - g.ph; w0 = wo * g.sw - g.pw;
    }
#pragma unroll
    for (int e = 0; e < RA; ++e) {
      const int co = co0 + 4 * (cq + 8 * e);
      ra[e] = (min_ && co < g.N) ? *reinterpret_cast<const f32x4*>(dy + (int64_t)m * g.N + co) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int e = 0; e < RB; ++e) {
      const int ti = t0 + dt[e], hi = h0 + dh[e], wi = w0 + dw[e];
      if (min_ && kin[e] && (unsigned)ti < (unsigned)g.Ti && (unsigned)hi < (unsigned)g.Hi && (unsigned)wi < (unsigned)g.Wi)
        rb[e] = *reinterpret_cast<const f32x4*>(x + xb + (((int64_t)ti * g.Hi + hi) * g.Wi + wi) * g.C + cc[e]);
      else
        rb[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (s_begin < s_end) load_slab(s_begin);
  for (int slab = s_begin; slab < s_end; ++slab) {
#pragma unroll
    for (int e = 0; e < RA; ++e)
#pragma unroll
      for (int j = 0; j < 4; ++j) As[4 * (cq + 8 * e) + j][mr] = ra[e][j];
#pragma unroll
    for (int e = 0; e < RB; ++e)
#pragma unroll
      for (int j = 0; j < 4; ++j) Bs[4 * (cq + 8 * e) + j][mr] = rb[e][j];
    __syncthreads();
    if (slab + 1 < s_end) load_slab(slab + 1);
    f32x4 a[MI][2], b[NJ][2];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      a[i][0] = *reinterpret_cast<const f32x4*>(&As[wm + 16 * i + li][8 * lg]);
      a[i][1] = *reinterpret_cast<const f32x4*>(&As[wm + 16 * i + li][8 * lg + 4]);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      b[j][0] = *reinterpret_cast<const f32x4*>(&Bs[wn + 16 * j + li][8 * lg]);
      b[j][1] = *reinterpret_cast<const f32x4*>(&Bs[wn + 16 * j + li][8 * lg + 4]);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s >> 2][s & 3], b[j][s >> 2][s & 3], acc[i][j], 0, 0, 0);
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int k = k0 + wn + 16 * j + li;
    if (k >= g.K) continue;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = co0 + wm + 16 * i + 4 * lg + q;
        if (co < g.N) part[(int64_t)co * g.K + k] = acc[i][j][q];
      }
  }
}

// wgrad finish: dw[co][ci][tap] (+)= sc[co] · Σ_z part[z][co][tap·C + ci], ci < Cin_w (padded channels dropped)
__global__ __launch_bounds__(256) void conv3d_wgrad_finish_kernel(const float* __restrict__ part, int splits, int N, int K, int C, int Cin_w, int taps,
                                                                  const float* __restrict__ scale, const float* __restrict__ bn_w,
                                                                  const float* __restrict__ bn_var, float eps, int accumulate, float* __restrict__ dw) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)N * Cin_w * taps) return;
  const int tap = (int)(idx % taps);
  const int64_t r = idx / taps;
  const int ci = (int)(r % Cin_w);
  const int co = (int)(r / Cin_w);
  const int64_t src = (int64_t)co * K + (int64_t)tap * C + ci;
  const int64_t slab = (int64_t)N * K;
  float v = 0.f;
  for (int z = 0; z < splits; ++z) v += part[z * slab + src];
  if (bn_w) v *= bn_w[co] / sqrtf(bn_var[co] + eps);
  else if (scale) v *= scale[co];
  dw[idx] = accumulate ? dw[idx] + v : v;
}

// MaxPool3d(3, 2, 1) forward that also records the argmax (0..26, first maximum in scan order, as torch) of every output
__global__ __launch_bounds__(256) void maxpool3d_argmax_kernel(const float* __restrict__ x, int B, int T, int H, int W, int C, int To, int Ho, int Wo,
                                                               float* __restrict__ y, uint8_t* __restrict__ am) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * To * Ho * Wo * C) return;
  const int c = (int)(idx % C);
  int64_t q = idx / C;
  const int wo = (int)(q % Wo); q /= Wo;
  const int ho = (int)(q % Ho); q /= Ho;
  const int to = (int)(q % To);
  const int64_t b = q / To;
  float m = -INFINITY;
  int best = 0;
  bool first = true;
  for (int dt = 0; dt < 3; ++dt) {
    const int t = 2 * to - 1 + dt;
    if ((unsigned)t >= (unsigned)T) continue;
    for (int dh = 0; dh < 3; ++dh) {
      const int h = 2 * ho - 1 + dh;
      if ((unsigned)h >= (unsigned)H) continue;
      for (int dw = 0; dw < 3; ++dw) {
        const int ww = 2 * wo - 1 + dw;
        if ((unsigned)ww >= (unsigned)W) continue;
        const float v = x[(((b * T + t) * H + h) * W + ww) * C + c];
        if (first || v > m) { best = (dt * 3 + dh) * 3 + dw; }  // strict: the first maximum keeps its place
        m = fmaxf(m, v);                                           // the value exactly as maxpool3d_ndhwc_kernel forms it
        first = false;
      }
    }
  }
  y[idx] = m;
  am[idx] = (uint8_t)best;
}

// MaxPool3d backward as a gather: every input element sums, in window scan order, the gradients of the (at most 8) windows whose
// argmax it is; then 0 unless mask[x] > 0 (NULL: no mask — the stem's ReLU mask is passed here)
__global__ __launch_bounds__(256) void maxpool3d_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ am, int B, int T, int H, int W, int C,
                                                            int To, int Ho, int Wo, const float* __restrict__ mask, float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * T * H * W * C) return;
  const int c = (int)(idx % C);
  int64_t q = idx / C;
  const int w = (int)(q % W); q /= W;
  const int h = (int)(q % H); q /= H;
  const int t = (int)(q % T);
  const int64_t b = q / T;
  float v = 0.f;
  if (!mask || mask[idx] > 0.f) {
    // window o covers input i when 2o - 1 <= i <= 2o + 1: o in [(i) / 2, (i + 1) / 2]
    for (int to = t / 2; to <= (t + 1) / 2 && to < To; ++to)
      for (int ho = h / 2; ho <= (h + 1) / 2 && ho < Ho; ++ho)
        for (int wo = w / 2; wo <= (w + 1) / 2 && wo < Wo; ++wo) {
          const int pos = ((t - 2 * to + 1) * 3 + (h - 2 * ho + 1)) * 3 + (w - 2 * wo + 1);
          const int64_t o = (((b * To + to) * Ho + ho) * Wo + wo) * C + c;
          if (am[o] == pos) v += dy[o];
        }
  }
  dx[idx] = v;
}

// gradient entering the trunk at its last block output y (B, P, C) NDHWC, masked by y > 0 (the last ReLU):
// from dpooled (B, C): dpooled / P at every position; from dfeatures (B, C, P) NCDHW: its transpose
__global__ __launch_bounds__(256) void r3d_grad_in_kernel(const float* __restrict__ dpooled, const float* __restrict__ dfeat, const float* __restrict__ y,
                                                          int64_t B, int P, int C, float* __restrict__ g) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * P * C) return;
  const int c = (int)(idx % C);
  const int64_t r = idx / C;
  const int p = (int)(r % P);
  const int64_t b = r / P;
  float v = dpooled ? dpooled[b * C + c] / (float)P : dfeat[(b * C + c) * P + p];
  g[idx] = y[idx] > 0.f ? v : 0.f;
}

// ---- thin-input data gradient: the stem (c_in <= 4 stored as 4, 7x7x7, stride (1, 2, 2), pad 3) ----
// Forward: y[b, to, ho, wo, co] = Σ x[b, to + dt - 3, 2·ho + dh - 3, 2·wo + dw - 3, ci] · w[co, ci, dt, dh, dw].  For the input position
// (t, h = 2i + a, w = 2j + b) the taps with 2 | (a + 3 - dh) and 2 | (b + 3 - dw) reach dy at to = t - 3 + jt (jt = 6 - dt, 0..6),
// ho = i - 1 + jh (dh = a + 5 - 2·jh, jh 0..3) and wo = j - 1 + jw (dw = b + 5 - 2·jw): the four (a, b) classes of a 2x2 block read the
// SAME 7x4x4 dy window.  So one row of the matrix tile is a block (b, t, i, j), its 16 columns are (a, b, ci), and the contraction
// k = (jt, jh, jw, co) is 112·c_out long; taps a class does not have (dh = -1: jh = 3 of a = 0; likewise jw = 3 of b = 0) and the
// padded channel are zeros in the repacked weight ([jt][jh][jw][co / 4][column][co % 4], 1792·c_out floats).
// A workgroup (4 waves) owns TH_TI x TH_TJ = 8 x 16 blocks of one (b, t): wave v the rows il = 2v, 2v + 1, one 16 x 16 MFMA block each
// (its 16 rows are the 16 consecutive j).  Per temporal tap the dy window (11 x 19 positions x up to 64 channels) is staged ONCE into
// LDS — positions outside dy as zeros — and the MFMA A operand is read straight from it at ((il + jh), (jl + jw)): no im2col copy.  The
// weight streams through LDS by (jt, jh) (4 jw x 64 co x 16 columns = 16 KB).  76.6 KB of LDS: two workgroups per CU, one staging
// while the other multiplies.  Pitch 72 floats: row li's 16-byte slot is 18·li + lg (mod 16: 2·li + lg), distinct over each
// ds_read_b128 lane group; the weight's slot is 16·(4g + lg) + li, distinct as well.  c_out above 64 runs in channel chunks of 64
// (the last one short, zero-filled to a multiple of 16), in order: one thread, one fixed summation order per dx element.
constexpr int TH_TI = 8, TH_TJ = 16;
constexpr int TH_WI = TH_TI + 3, TH_WJ = TH_TJ + 3;
constexpr int TH_CB = 64;               // channels of dy per chunk
constexpr int TH_P = TH_CB + 8;         // window pitch (floats)
constexpr int TH_WIN = TH_WI * TH_WJ * TH_P;          // floats
constexpr int TH_WS = 4 * (TH_CB / 4) * 16 * 4;       // floats: [jw][co quad][column][4]
constexpr int TH_LDS_BYTES = (TH_WIN + TH_WS) * (int)sizeof(float);

struct ThinGeom {
  int B, T, H, W;          // dx
  int To, Ho, Wo, N;       // dy (B, To, Ho, Wo, N), N = c_out
  int c_in;                // real channels (<= 4)
  int tiles_i, tiles_j;
};

template <bool NCDHW>
__global__ __launch_bounds__(256, 2) void conv3d_dgrad_thin_kernel(const float* __restrict__ dy, const float* __restrict__ wt, ThinGeom g,
                                                                   float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float th_lds[];
  float* win = th_lds;
  float* wS = th_lds + TH_WIN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  int q = blockIdx.x;
  const int tj = q % g.tiles_j; q /= g.tiles_j;
  const int ti = q % g.tiles_i; q /= g.tiles_i;
  const int t = q % g.T;
  const int b = q / g.T;
  const int i0 = ti * TH_TI, j0 = tj * TH_TJ;
  const int nq_all = g.N / 4;  // channel quads of dy

  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int co0 = 0; co0 < g.N; co0 += TH_CB) {
    const int cb = min(TH_CB, g.N - co0);         // real channels of this chunk (a multiple of 4)
    const int cbq = cb / 4, cbq_pad = (cb + 15) / 16 * 4;  // quads staged: zero-filled up to a multiple of 16 channels
    for (int jt = 0; jt < 7; ++jt) {
      const int to = t - 3 + jt;
      if ((unsigned)to >= (unsigned)g.To) continue;  // the whole temporal tap lies outside dy (uniform over the workgroup)
      __syncthreads();  // the previous tap's reads of the window are done
      for (int idx = tid; idx < TH_WI * TH_WJ * cbq_pad; idx += 256) {
        const int cq = idx % cbq_pad, pos = idx / cbq_pad;
        const int wj = pos % TH_WJ, wi = pos / TH_WJ;
        const int ho = i0 - 1 + wi, wo = j0 - 1 + wj;
        f32x4 v{0.f, 0.f, 0.f, 0.f};
        if (cq < cbq && (unsigned)ho < (unsigned)g.Ho && (unsigned)wo < (unsigned)g.Wo)
          v = *reinterpret_cast<const f32x4*>(dy + ((((int64_t)b * g.To + to) * g.Ho + ho) * g.Wo + wo) * g.N + co0 + 4 * cq);
        *reinterpret_cast<f32x4*>(win + pos * TH_P + 4 * cq) = v;
      }
      for (int jh = 0; jh < 4; ++jh) {
        if (jh) __syncthreads();  // the previous (jt, jh)'s reads of the weight are done (jh = 0: the barrier above)
        for (int idx = tid; idx < 4 * cbq_pad * 16; idx += 256) {
          const int col = idx & 15, cq = (idx >> 4) % cbq_pad, jw = (idx >> 4) / cbq_pad;
          f32x4 v{0.f, 0.f, 0.f, 0.f};
          if (cq < cbq) v = *reinterpret_cast<const f32x4*>(wt + ((((int64_t)(jt * 4 + jh) * 4 + jw) * nq_all + co0 / 4 + cq) * 16 + col) * 4);
          *reinterpret_cast<f32x4*>(wS + ((jw * (TH_CB / 4) + cq) * 16 + col) * 4) = v;
        }
        __syncthreads();
        const float* a0 = win + ((2 * wave + jh) * TH_WJ + li) * TH_P + 4 * lg;
        const float* a1 = a0 + TH_WJ * TH_P;
        const float* bp = wS + (lg * 16 + li) * 4;
        for (int jw = 0; jw < 4; ++jw)
          for (int gq = 0; gq < cbq_pad / 4; ++gq) {
            const f32x4 va = *reinterpret_cast<const f32x4*>(a0 + jw * TH_P + 16 * gq);
            const f32x4 vb = *reinterpret_cast<const f32x4*>(a1 + jw * TH_P + 16 * gq);
            const f32x4 vw = *reinterpret_cast<const f32x4*>(bp + (jw * (TH_CB / 4) + 4 * gq) * 64);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[s], vw[s], acc[0], 0, 0, 0);
              acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[s], vw[s], acc[1], 0, 0, 0);
            }
          }
      }
    }
  }

  // lane (li, lg), register e: row jl = 4·lg + e of the wave's block r, column li = (2a + b)·4 + ci
  const int ci = li & 3, pb = (li >> 2) & 1, pa = li >> 3;
  if (NCDHW && ci >= g.c_in) return;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int h = 2 * (i0 + 2 * wave + r) + pa;
    if (h >= g.H) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int w = 2 * (j0 + 4 * lg + e) + pb;
      if (w >= g.W) continue;
      if (NCDHW)
        dx[((((int64_t)b * g.c_in + ci) * g.T + t) * g.H + h) * g.W + w] = acc[r][e];
      else
        dx[((((int64_t)b * g.T + t) * g.H + h) * g.W + w) * 4 + ci] = ci < g.c_in ? acc[r][e] : 0.f;
    }
  }
}

// the thin copy, walked in destination order ([jt][jh][jw][co / 4][column][co % 4])
__global__ __launch_bounds__(256) void conv3d_repack_dgrad_thin_kernel(const float* __restrict__ w, int Cout, int Cin, const float* __restrict__ scale,
                                                                       float* __restrict__ out) {
  const int n = 1792 * Cout;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
    int q = idx;
    const int e = q & 3; q >>= 2;
    const int col = q & 15; q >>= 4;
    const int cq = q % (Cout / 4); q /= Cout / 4;
    const int jw = q & 3; q >>= 2;
    const int jh = q & 3;
    const int jt = q >> 2;
    const int co = 4 * cq + e, ci = col & 3, pb = (col >> 2) & 1, pa = col >> 3;
    const int dt = 6 - jt, dh = pa + 5 - 2 * jh, dw = pb + 5 - 2 * jw;
    float v = 0.f;
    if (ci < Cin && dh >= 0 && dw >= 0) v = (scale ? scale[co] : 1.f) * w[(((int64_t)co * Cin + ci) * 7 + dt) * 49 + dh * 7 + dw];
    out[idx] = v;
  }
}

// the one geometry of the thin data gradient; c_in is the forward conv's REAL channel count (<= 4)
int check_thin_desc(const stlt_conv3d_desc* d, const char* who, ThinGeom* g) {
  if (!d) return stlt_set_error(STLT_EINVAL, "%s: null descriptor", who);
  if (d->B <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->c_out <= 0 || d->c_in <= 0 || d->T > (1 << 24) || d->H > (1 << 24) || d->W > (1 << 24) ||
      d->c_out > (1 << 16))
    return stlt_set_error(STLT_EINVAL, "%s: sizes must be positive (c_out at most 65536)", who);
  if (d->c_in > 4) return stlt_set_error(STLT_EINVAL, "%s: the thin data gradient takes at most 4 input channels, got %lld (stlt_conv3d_bwd_data serves wider inputs)", who, (long long)d->c_in);
  if (d->st != 1 || d->sh != 2 || d->sw != 2)
    return stlt_set_error(STLT_EINVAL, "%s: the thin data gradient is built for stride (1, 2, 2) only, got (%lld, %lld, %lld)", who, (long long)d->st,
                          (long long)d->sh, (long long)d->sw);
  if (d->kt != 7 || d->kh != 7 || d->kw != 7 || d->pt != 3 || d->ph != 3 || d->pw != 3)
    return stlt_set_error(STLT_EINVAL, "%s: the thin data gradient is built for kernel 7x7x7 with padding 3 only", who);
  if (d->c_out % 4) return stlt_set_error(STLT_EINVAL, "%s: c_out must be a multiple of 4 (dy's rows are read as 16-byte quads), got %lld", who, (long long)d->c_out);
  const int64_t To = d->T, Ho = (d->H - 1) / 2 + 1, Wo = (d->W - 1) / 2 + 1;
  const int64_t tiles_i = cdiv(Ho, TH_TI), tiles_j = cdiv(Wo, TH_TJ);
  if (prod_over({d->B, d->T, tiles_i, tiles_j}, 0x7fffff00LL) || prod_over({d->B, d->T, d->H, d->W, 4}, 1LL << 40) || prod_over({d->B, To, Ho, Wo, d->c_out}, 1LL << 40))
    return stlt_set_error(STLT_EINVAL, "%s: shape too large", who);
  if (g) *g = ThinGeom{(int)d->B, (int)d->T, (int)d->H, (int)d->W, (int)To, (int)Ho, (int)Wo, (int)d->c_out, (int)d->c_in, (int)tiles_i, (int)tiles_j};
  return 0;
}

int launch_dgrad_thin(const ThinGeom& g, const float* dy, const float* wt, float* dx, int ncdhw, hipStream_t s) {
  StltProfScope ps(STLT_K_CONV_DGRAD_THIN, s);
  static StltPerDeviceInt attr_set;
  int& set = attr_set.ref();
  if (!set) {
    if (hipError_t e = hipFuncSetAttribute((const void*)conv3d_dgrad_thin_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, TH_LDS_BYTES); e != hipSuccess)
      return stlt_set_error((int)e, "conv3d_dgrad_thin: hipFuncSetAttribute: %s", hipGetErrorString(e));
    if (hipError_t e = hipFuncSetAttribute((const void*)conv3d_dgrad_thin_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, TH_LDS_BYTES); e != hipSuccess)
      return stlt_set_error((int)e, "conv3d_dgrad_thin: hipFuncSetAttribute: %s", hipGetErrorString(e));
    set = 1;
  }
  const int64_t wgs = (int64_t)g.B * g.T * g.tiles_i * g.tiles_j;
  // the formulation's FLOPs, zero taps and the padded channel included: rows (2x2 blocks, whole tiles) x 16 columns x 112·c_out
  const double flops = 2.0 * (double)wgs * (TH_TI * TH_TJ) * 16.0 * 112.0 * g.N;
  stlt_prof_note("dgrad_thin B=%d T=%d H=%d W=%d c_out=%d %s wgs=%lld", g.B, g.T, g.H, g.W, g.N, ncdhw ? "ncdhw" : "ndhwc", (long long)wgs);
  stlt_prof_note_flops(flops);
  const dim3 grid((unsigned)wgs), block(256);
  if (ncdhw)
    hipLaunchKernelGGL(conv3d_dgrad_thin_kernel<true>, grid, block, TH_LDS_BYTES, s, dy, wt, g, dx);
  else
    hipLaunchKernelGGL(conv3d_dgrad_thin_kernel<false>, grid, block, TH_LDS_BYTES, s, dy, wt, g, dx);
  return stlt_check_launch("conv3d_dgrad_thin_kernel");
}

// ---- host plans ----
struct SubConv { ConvGeom g; DgEpi e; int64_t w_off; };

// the parity classes of a dgrad (forward geometry f, f.C = c_in of the forward conv, f.N = c_out); sc/mask/add per DgEpi
int dgrad_plan(const ConvGeom& f, SubConv* out) {
  int n = 0;
  int64_t off = 0;
  for (int a = 0; a < f.st; ++a)
    for (int b = 0; b < f.sh; ++b)
      for (int c = 0; c < f.sw; ++c) {
        int k1, k2, k3, p1, p2, p3;
        sub_dims(f.kt, f.st, f.pt, a, &k1, &p1);
        sub_dims(f.kh, f.sh, f.ph, b, &k2, &p2);
        sub_dims(f.kw, f.sw, f.pw, c, &k3, &p3);
        const int nt = f.Ti > a ? (f.Ti - a + f.st - 1) / f.st : 0, nh = f.Hi > b ? (f.Hi - b + f.sh - 1) / f.sh : 0,
                  nw = f.Wi > c ? (f.Wi - c + f.sw - 1) / f.sw : 0;
        SubConv& s = out[n++];
        // input of the sub-conv: dy (B, To, Ho, Wo, N); output: class rows (B, nt, nh, nw, C)
        const bool empty = k1 == 0 || k2 == 0 || k3 == 0;
        // row a reads dy at a - p' + j (a stride-1 conv with padding p'); a class without taps has K = 0 (its rows get the epilogue alone)
        s.g = ConvGeom{f.B, f.To, f.Ho, f.Wo, f.N, nt, nh, nw, f.C, empty ? 1 : k1, empty ? 1 : k2, empty ? 1 : k3, 1, 1, 1, p1, p2, p3,
                       f.B * nt * nh * nw, empty ? 0 : k1 * k2 * k3 * f.N};
        s.e = DgEpi{nullptr, nullptr, nullptr, f.Ti, f.Hi, f.Wi, f.st, a, b, c};
        s.w_off = off;
        off += (int64_t)(empty ? 0 : k1 * k2 * k3) * f.N * f.C;
      }
  return n;
}

// what the data gradient asks beyond check_desc: at most 2^3 parity classes (SubConv[8]), and a contraction, taps · c_out, that is an int
bool dgrad_fits(const ConvGeom& g) { return g.st <= 2 && g.sh <= 2 && g.sw <= 2 && !prod_over({g.kt, g.kh, g.kw, g.N}, 0x7fffff00LL); }

// a class without taps (K = 0) or without rows (M = 0: an input extent of 1 under stride 2) is never split
int64_t dgrad_splits(const ConvGeom& s) { return s.K > 0 && s.M > 0 ? conv_plan_splits(s.M, s.N, s.K) : 1; }

int64_t dgrad_ws_bytes(const ConvGeom& f) {
  SubConv sub[8];
  const int n = dgrad_plan(f, sub);
  int64_t mx = 0;
  for (int i = 0; i < n; ++i) mx = std::max(mx, conv_split_bytes(sub[i].g, dgrad_splits(sub[i].g)));
  return mx;
}

// skip_empty: leave the rows of tap-less classes as they are (the caller's dx already holds add, masked: an in-place add-source)
int launch_dgrad(const ConvGeom& f, const float* dy, const float* wd, const float* sc, const float* mask, const float* add, float* dx, float* part,
                 int64_t part_bytes, int n_split, hipStream_t s, bool skip_empty = false) {
  if (f.st != f.sh || f.st != f.sw) {
    // mixed strides: os differs per dimension, which DgEpi does not carry
    return stlt_set_error(STLT_EINVAL, "conv3d backward: the data gradient needs equal strides in t, h and w, got (%d, %d, %d)", f.st, f.sh, f.sw);
  }
  SubConv sub[8];
  const int n = dgrad_plan(f, sub);
  for (int i = 0; i < n; ++i) {
    SubConv& c = sub[i];
    if (c.g.M == 0 || (skip_empty && c.g.K == 0)) continue;
    c.e.sc = sc; c.e.mask = mask; c.e.add = add;
    const int bn = conv_bn_tile(c.g.N);
    const auto [splits, per] = split_ranges(cdiv(c.g.K, CK), n_split > 0 ? n_split : dgrad_splits(c.g));
    if (splits > 1 && (!part || part_bytes < conv_split_bytes(c.g, splits)))
      return stlt_set_error(STLT_EWORKSPACE, "stlt_conv3d_bwd_data: %lld splits need %lld workspace bytes, %lld lent", (long long)splits,
                            (long long)conv_split_bytes(c.g, splits), (long long)part_bytes);
    const dim3 grid((unsigned)cdiv(c.g.M, BM), (unsigned)cdiv(c.g.N, bn), (unsigned)splits), block(256);
    const float* w = wd + c.w_off;
    if (splits == 1) {
      if (bn == 64)
        hipLaunchKernelGGL((conv3d_igemm_kernel<64, true>), grid, block, 0, s, dy, w, c.g, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, 0, dx, (int)per, c.e);
      else
        hipLaunchKernelGGL((conv3d_igemm_kernel<128, true>), grid, block, 0, s, dy, w, c.g, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, 0, dx, (int)per, c.e);
      if (int e = stlt_check_launch("conv3d_igemm_kernel<bwd>")) return e;
    } else {
      if (bn == 64)
        hipLaunchKernelGGL((conv3d_igemm_kernel<64, true>), grid, block, 0, s, dy, w, c.g, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, 0, part, (int)per, c.e);
      else
        hipLaunchKernelGGL((conv3d_igemm_kernel<128, true>), grid, block, 0, s, dy, w, c.g, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, 0, part, (int)per, c.e);
      if (int e = stlt_check_launch("conv3d_igemm_kernel<bwd>")) return e;
      hipLaunchKernelGGL(conv3d_dgrad_finish_kernel, dim3((unsigned)cdiv((int64_t)c.g.M * c.g.N, 256)), dim3(256), 0, s, part, (int)splits, c.g, c.e, dx);
      if (int e = stlt_check_launch("conv3d_dgrad_finish_kernel")) return e;
    }
  }
  return 0;
}

inline int wgrad_tile(int64_t N) { return N <= 64 ? 64 : 128; }

int64_t wgrad_plan_splits(const ConvGeom& g) {
  const int64_t tiles = cdiv(g.N, wgrad_tile(g.N)) * cdiv(g.K, WG_TK);
  const int64_t slabs = cdiv(g.M, CK);
  int64_t splits = cdiv(WG_TARGET_WG, tiles);
  splits = std::min(splits, slabs / WG_MIN_SLABS);
  splits = std::min(splits, WG_SPLIT_MAX);
  return split_ranges(slabs, splits).splits;
}

// the weight gradient's partial slabs hold c_out · K floats each: past 2^40 of them the byte count of WG_SPLIT_MAX slabs leaves int64
bool wgrad_fits(const ConvGeom& g) { return !prod_over({g.N, g.K}, 1LL << 40); }

int64_t wgrad_ws_bytes(const ConvGeom& g, int64_t splits) { return splits * (int64_t)g.N * g.K * (int64_t)sizeof(float); }

int launch_wgrad(const ConvGeom& g, const float* x, const float* dy, int cin_w, const float* scale, const float* bn_w, const float* bn_var, float eps,
                 int accumulate, float* dw, int64_t want_splits, float* part, hipStream_t s) {
  const auto [splits, per] = split_ranges(cdiv(g.M, CK), want_splits);
  const int ta = wgrad_tile(g.N);
  const dim3 grid((unsigned)cdiv(g.N, ta), (unsigned)cdiv(g.K, WG_TK), (unsigned)splits), block(256);
  if (ta == 64)
    hipLaunchKernelGGL(conv3d_wgrad_kernel<64>, grid, block, 0, s, x, dy, g, part, (int)per);
  else
    hipLaunchKernelGGL(conv3d_wgrad_kernel<128>, grid, block, 0, s, x, dy, g, part, (int)per);
  if (int e = stlt_check_launch("conv3d_wgrad_kernel")) return e;
  const int taps = g.kt * g.kh * g.kw;
  hipLaunchKernelGGL(conv3d_wgrad_finish_kernel, dim3((unsigned)cdiv((int64_t)g.N * cin_w * taps, 256)), dim3(256), 0, s, part, (int)splits, g.N, g.K, g.C,
                     cin_w, taps, scale, bn_w, bn_var, eps, accumulate, dw);
  return stlt_check_launch("conv3d_wgrad_finish_kernel");
}

// ---- the whole trunk, stated once.  trunk_plan is the only function that knows R3D-50's structure: it walks r3d_conv_meta's table
// (the stem; per block conv1, conv2, conv3 and, in a layer's first block, the downsample) through check_desc and lays out the three
// buffers.  The size queries return its byte counts; the forward and the reverse sweep add its offsets to the caller's bases.
//   inference workspace  [xin][X0][X1][DS][T1 | T2][part]   X0 / X1: the block outputs, ping-pong (X0 first holds the max-pool's);
//                        T1 / T2: conv1's / conv2's (T1 first holds the stem's); DS: the downsample's; part: split-forward partials
//   tape                 [xin][stem][pool][argmax], then per block [conv1][conv2][output]
//   backward workspace   [G3][G2][G1][GX][GS][part]          gradients at a block's output, conv2, conv1 and input; GS: at the stem's
//                        output; part: the largest weight- or data-gradient partial
constexpr int R3D_LAYERS = 4;                                       // each opens with the one block that has a downsample
constexpr int R3D_NBLOCKS = (STLT_R3D_CONVS - 1 - R3D_LAYERS) / 3;  // 53 = the stem + 3 per block + a downsample per layer

struct TrunkBlock {
  int conv1;             // conv1's index; conv2, conv3 and (ds) the downsample follow it in state-dict order
  bool ds;
  int64_t x, a1, a2, y;  // tape slots: the block's input (the block before's output; the first block's: the max-pool's), conv1, conv2, output
};

struct TrunkPlan {
  ConvGeom g[STLT_R3D_CONVS];
  int64_t fwd_splits[STLT_R3D_CONVS];
  TrunkBlock blk[R3D_NBLOCKS];
  int64_t stem_elems, pool_elems, act_elems;  // act: the largest block-level activation
  int64_t fwd_part_bytes, bwd_part_bytes;     // the largest split-forward partial; the largest dgrad / wgrad partial
  struct { int64_t xin, stem, pool, argmax, bytes; } tape;  // byte offsets; the blocks' slots are in blk[]
  struct { int64_t xin, x[2], ds, t1, t2, part, bytes; } ws;
  struct { int64_t g3, g2, g1, gx, gs, part, bytes; } bws;
};

struct Carver {  // consecutive 256-byte aligned buffers
  int64_t off = 0;
  int64_t take(int64_t bytes) { const int64_t o = off; off += (int64_t)stlt_align256((size_t)bytes); return o; }
};

bool trunk_plan(int64_t B, int64_t T, int64_t H, int64_t W, TrunkPlan* P) {
  TrunkPlan& p = *P;
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || T > 4096 || H > 4096 || W > 4096 || B > (1 << 20)) return false;
  const int64_t f = sizeof(float);
  // conv i over an input of (t, h, w): the table's cubic kernel with padding k / 2, channels stored in quads, stride s (the stem: 1 in t)
  auto geom = [&](int i, int64_t t, int64_t h, int64_t w) -> bool {
    const R3dConvMeta m = r3d_conv_meta(i);
    const int64_t pad = m.k / 2;
    const stlt_conv3d_desc d{B, t, h, w, (m.cin + 3) / 4 * 4, m.cout, m.k, m.k, m.k, i == 0 ? 1 : m.s, m.s, m.s, pad, pad, pad};
    if (check_desc(&d, &p.g[i])) return false;
    p.fwd_splits[i] = conv_plan_splits(p.g[i].M, p.g[i].N, p.g[i].K);
    return true;
  };
  auto elems = [&](int i) { return (int64_t)p.g[i].M * p.g[i].N; };
  if (!geom(0, T, H, W)) return false;
  const ConvGeom& s0 = p.g[0];
  const int64_t Tp = out_dim(s0.To, 3, 2, 1), Hp = out_dim(s0.Ho, 3, 2, 1), Wp = out_dim(s0.Wo, 3, 2, 1);  // the max-pool
  p.stem_elems = elems(0);
  p.pool_elems = B * Tp * Hp * Wp * s0.N;
  Carver tape;
  p.tape.xin = tape.take(B * T * H * W * 4 * f);
  p.tape.stem = tape.take(p.stem_elems * f);
  p.tape.pool = tape.take(p.pool_elems * f);
  p.tape.argmax = tape.take(p.pool_elems);
  p.act_elems = p.pool_elems;
  int64_t t = Tp, h = Hp, w = Wp, x = p.tape.pool;
  int i = 1;
  for (TrunkBlock& k : p.blk) {
    k.conv1 = i;
    k.ds = r3d_conv_meta(i + 3).cout == r3d_conv_meta(i + 2).cout;  // the entry behind conv3 projects onto this block's output: its downsample
    if (!geom(i, t, h, w) || !geom(i + 1, p.g[i].To, p.g[i].Ho, p.g[i].Wo) || !geom(i + 2, p.g[i + 1].To, p.g[i + 1].Ho, p.g[i + 1].Wo)) return false;
    if (k.ds && !geom(i + 3, t, h, w)) return false;
    k.x = x;
    k.a1 = tape.take(elems(i) * f);
    k.a2 = tape.take(elems(i + 1) * f);
    k.y = tape.take(elems(i + 2) * f);
    p.act_elems = std::max({p.act_elems, elems(i), elems(i + 1), elems(i + 2)});
    t = p.g[i + 2].To; h = p.g[i + 2].Ho; w = p.g[i + 2].Wo; x = k.y;
    i += k.ds ? 4 : 3;
  }
  p.tape.bytes = tape.off;
  p.fwd_part_bytes = p.bwd_part_bytes = 0;
  for (int c = 0; c < STLT_R3D_CONVS; ++c) {
    p.fwd_part_bytes = std::max(p.fwd_part_bytes, conv_split_bytes(p.g[c], p.fwd_splits[c]));
    p.bwd_part_bytes = std::max(p.bwd_part_bytes, wgrad_ws_bytes(p.g[c], wgrad_plan_splits(p.g[c])));
    if (c > 0) p.bwd_part_bytes = std::max(p.bwd_part_bytes, dgrad_ws_bytes(p.g[c]));  // the stem's data gradient is the thin kernel: no scratch
  }
  Carver ws;
  p.ws.xin = ws.take(B * T * H * W * 4 * f);
  p.ws.x[0] = ws.take(p.act_elems * f);
  p.ws.x[1] = ws.take(p.act_elems * f);
  p.ws.ds = ws.take(p.act_elems * f);
  p.ws.t1 = ws.take(std::max(p.stem_elems, 2 * p.act_elems) * f);  // one region: the stem's output is dead once the blocks write T1 and T2
  p.ws.t2 = p.ws.t1 + p.act_elems * f;
  p.ws.part = ws.take(p.fwd_part_bytes);
  p.ws.bytes = ws.off;
  Carver bws;
  p.bws.g3 = bws.take(p.act_elems * f);
  p.bws.g2 = bws.take(p.act_elems * f);
  p.bws.g1 = bws.take(p.act_elems * f);
  p.bws.gx = bws.take(p.act_elems * f);
  p.bws.gs = bws.take(p.stem_elems * f);
  p.bws.part = bws.take(p.bwd_part_bytes);
  p.bws.bytes = bws.off;
  return true;
}

int check_r3d_params(const stlt_r3d_params* p, const char* who) {
  if (!p) return stlt_set_error(STLT_EINVAL, "%s: null parameters", who);
  for (int i = 0; i < STLT_R3D_CONVS; ++i) {
    const stlt_r3d_conv& c = p->conv[i];
    if (!c.w || !c.bn_w || !c.bn_b || !c.bn_mean || !c.bn_var) return stlt_set_error(STLT_EINVAL, "%s: conv %d has a null weight or BatchNorm buffer", who, i);
    if ((uintptr_t)c.w & 15) return stlt_set_error(STLT_EINVAL, "%s: packed weight %d is not 16-byte aligned", who, i);
  }
  return 0;
}

// the first block of stage `layer` (1 .. R3D_LAYERS: the layer-th block with a downsample); R3D_LAYERS + 1: one past the last block
int stage_first_block(const TrunkPlan& P, int layer) {
  int seen = 0;
  for (int b = 0; b < R3D_NBLOCKS; ++b)
    if (P.blk[b].ds && ++seen == layer) return b;
  return R3D_NBLOCKS;
}

}  // namespace

extern "C" {

size_t stlt_conv3d_bwd_data_workspace_bytes(const stlt_conv3d_desc* d, int n_split) {
  ConvGeom g;
  if (check_desc(d, &g) || !dgrad_fits(g)) return 0;
  if (n_split <= 0) return (size_t)dgrad_ws_bytes(g);
  SubConv sub[8];
  const int n = dgrad_plan(g, sub);
  int64_t mx = 0;
  for (int i = 0; i < n; ++i)
    mx = std::max(mx, conv_split_bytes(sub[i].g, split_ranges(cdiv(sub[i].g.K, CK), n_split).splits));
  return (size_t)mx;
}

int stlt_conv3d_repack_dgrad(const float* w, const stlt_conv3d_desc* d, const float* scale, float* out, stlt_stream_t stream) {
  ConvGeom g;
  if (int e = check_desc(d, &g)) return e;
  if (!w || !out) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_repack_dgrad: null pointer");
  if (g.st > 2 || g.sh > 2 || g.sw > 2) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_repack_dgrad: strides above 2 are not supported");
  const int64_t n = (int64_t)g.N * g.C * g.kt * g.kh * g.kw;
  hipLaunchKernelGGL(conv3d_repack_dgrad_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, 256), 4096)), dim3(256), 0, (hipStream_t)stream, w, g.N, g.C,
                     g.kt, g.kh, g.kw, g.st, g.sh, g.sw, g.pt, g.ph, g.pw, scale, out);
  return stlt_check_launch("conv3d_repack_dgrad_kernel");
}

int stlt_conv3d_bwd_data(const stlt_conv3d_desc* d, const float* dy, const float* w_dgrad, const float* scale, const float* mask, const float* add,
                         int n_split, void* workspace, size_t workspace_bytes, float* dx, stlt_stream_t stream) {
  ConvGeom g;
  if (int e = check_desc(d, &g)) return e;
  if (!dy || !w_dgrad || !dx) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data: null pointer");
  if (g.N % 4) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data: c_out must be a multiple of 4 (it is the contraction's channel count), got %d", g.N);
  if (g.st > 2 || g.sh > 2 || g.sw > 2 || g.st != g.sh || g.st != g.sw)
    return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data: strides must be equal and at most 2");
  if (!dgrad_fits(g)) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data: shape too large");
  if (((uintptr_t)dy & 15) || ((uintptr_t)w_dgrad & 15)) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data: dy and w_dgrad must be 16-byte aligned");
  if (n_split < 0 || n_split > 1024) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data: n_split must lie in [0, 1024]");
  const size_t need = stlt_conv3d_bwd_data_workspace_bytes(d, n_split);
  if (need && (!workspace || workspace_bytes < need))
    return stlt_set_error(STLT_EWORKSPACE, "stlt_conv3d_bwd_data: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  return launch_dgrad(g, dy, w_dgrad, scale, mask, add, dx, (float*)workspace, (int64_t)workspace_bytes, n_split, (hipStream_t)stream);
}

size_t stlt_conv3d_bwd_weight_workspace_bytes(const stlt_conv3d_desc* d, int n_split) {
  ConvGeom g;
  if (check_desc(d, &g) || !wgrad_fits(g)) return 0;
  if (n_split < 0 || n_split > 4096) return 0;
  return (size_t)wgrad_ws_bytes(g, split_ranges(cdiv(g.M, CK), n_split == 0 ? wgrad_plan_splits(g) : n_split).splits);
}

int stlt_conv3d_bwd_weight(const stlt_conv3d_desc* d, const float* x, const float* dy, const float* scale, int64_t c_in_w, int accumulate, int n_split,
                           void* workspace, size_t workspace_bytes, float* dw, stlt_stream_t stream) {
  ConvGeom g;
  if (int e = check_desc(d, &g)) return e;
  if (!x || !dy || !dw) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_weight: null pointer");
  if (g.N % 4) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_weight: c_out must be a multiple of 4, got %d", g.N);
  if (!wgrad_fits(g)) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_weight: shape too large");
  if (c_in_w <= 0 || c_in_w > g.C) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_weight: c_in_w must lie in [1, c_in]");
  if (((uintptr_t)x & 15) || ((uintptr_t)dy & 15)) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_weight: x and dy must be 16-byte aligned");
  if (n_split < 0 || n_split > 4096) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_weight: n_split must lie in [0, 4096]");
  const size_t need = stlt_conv3d_bwd_weight_workspace_bytes(d, n_split);
  if (!workspace || workspace_bytes < need)
    return stlt_set_error(STLT_EWORKSPACE, "stlt_conv3d_bwd_weight: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int64_t splits = n_split == 0 ? wgrad_plan_splits(g) : n_split;
  return launch_wgrad(g, x, dy, (int)c_in_w, scale, nullptr, nullptr, 0.f, accumulate, dw, splits, (float*)workspace, (hipStream_t)stream);
}

int stlt_maxpool3d_ndhwc_train(const float* x, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, float* y, uint8_t* argmax, stlt_stream_t stream) {
  if (!x || !y || !argmax) return stlt_set_error(STLT_EINVAL, "stlt_maxpool3d_ndhwc_train: null pointer");
  if (int e = check_pool_shape("stlt_maxpool3d_ndhwc_train", B, T, H, W, C)) return e;
  const int64_t To = out_dim(T, 3, 2, 1), Ho = out_dim(H, 3, 2, 1), Wo = out_dim(W, 3, 2, 1);
  const int64_t n = B * To * Ho * Wo * C;
  if (n == 0) return 0;
  hipLaunchKernelGGL(maxpool3d_argmax_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, (int)B, (int)T, (int)H, (int)W, (int)C,
                     (int)To, (int)Ho, (int)Wo, y, argmax);
  return stlt_check_launch("maxpool3d_argmax_kernel");
}

int stlt_maxpool3d_ndhwc_bwd(const float* dy, const uint8_t* argmax, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, const float* mask, float* dx,
                             stlt_stream_t stream) {
  if (!dy || !argmax || !dx) return stlt_set_error(STLT_EINVAL, "stlt_maxpool3d_ndhwc_bwd: null pointer");
  if (int e = check_pool_shape("stlt_maxpool3d_ndhwc_bwd", B, T, H, W, C)) return e;
  const int64_t To = out_dim(T, 3, 2, 1), Ho = out_dim(H, 3, 2, 1), Wo = out_dim(W, 3, 2, 1);
  const int64_t n = B * T * H * W * C;
  if (n == 0) return 0;
  hipLaunchKernelGGL(maxpool3d_bwd_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dy, argmax, (int)B, (int)T, (int)H, (int)W,
                     (int)C, (int)To, (int)Ho, (int)Wo, mask, dx);
  return stlt_check_launch("maxpool3d_bwd_kernel");
}

// the whole-trunk size queries: the plan's byte counts (0 for a shape the plan refuses)
size_t stlt_r3d_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W) {
  TrunkPlan p;
  return trunk_plan(B, T, H, W, &p) ? (size_t)p.ws.bytes : 0;
}

size_t stlt_r3d_tape_bytes(int64_t B, int64_t T, int64_t H, int64_t W) {
  TrunkPlan p;
  return trunk_plan(B, T, H, W, &p) ? (size_t)p.tape.bytes : 0;
}

size_t stlt_r3d_backward_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W) {
  TrunkPlan p;
  return trunk_plan(B, T, H, W, &p) ? (size_t)p.bws.bytes : 0;
}

size_t stlt_r3d_backward_inputs_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W) {
  return stlt_r3d_backward_workspace_bytes(B, T, H, W);  // the thin data gradient needs no scratch of its own
}

int stlt_r3d_repack_all(const float* const* weights, const stlt_r3d_params* p, float* const* fwd, float* const* dgrad, stlt_stream_t stream) {
  if (!weights || !p || !fwd || !dgrad) return stlt_set_error(STLT_EINVAL, "stlt_r3d_repack_all: null pointer");
  R3dRepackArgs a;
  a.eps = p->bn_eps;
  for (int i = 0; i < STLT_R3D_CONVS; ++i) {
    if (!weights[i] || !p->conv[i].bn_w || !p->conv[i].bn_var || (!fwd[i] && !dgrad[i]))
      return stlt_set_error(STLT_EINVAL, "stlt_r3d_repack_all: conv %d has a null weight, BatchNorm buffer or destination", i);
    if (((uintptr_t)fwd[i] & 15) || (i > 0 && ((uintptr_t)dgrad[i] & 15)))
      return stlt_set_error(STLT_EINVAL, "stlt_r3d_repack_all: the copies of conv %d must be 16-byte aligned (the conv kernels load them as float4)", i);
    a.w[i] = weights[i]; a.bn_w[i] = p->conv[i].bn_w; a.bn_var[i] = p->conv[i].bn_var; a.fwd[i] = fwd[i]; a.dgrad[i] = i > 0 ? dgrad[i] : nullptr;
  }
  a.block0[0] = 0;
  for (int i = 0; i < STLT_R3D_CONVS; ++i) {
    int nf, nw;
    r3d_repack_counts(i, &nf, &nw);
    a.block0[i + 1] = a.block0[i] + (int)cdiv((int64_t)nf + nw, 256 * REPACK_ITEMS);
  }
  hipLaunchKernelGGL(r3d_repack_all_kernel, dim3((unsigned)a.block0[STLT_R3D_CONVS]), dim3(256), 0, (hipStream_t)stream, a);
  return stlt_check_launch("r3d_repack_all_kernel");
}

}  // extern "C"

// The trunk's forward, written once.  stlt_r3d_forward (tape == NULL) keeps its activations in the workspace's ping-pong buffers and
// runs the plain max-pool; stlt_r3d_train_forward writes every activation to its tape slot and runs the max-pool that records the
// argmax.  Nothing else differs, so the two give the same outputs bit for bit.
static int r3d_forward(const char* who, bool train, const stlt_r3d_params* p, const float* video, int64_t B, int64_t T, int64_t H, int64_t W, void* workspace,
                       size_t workspace_bytes, void* tape, size_t tape_bytes, float* features, float* pooled, stlt_stream_t stream) {
  if (int e = check_r3d_params(p, who)) return e;
  if (!video || (train && !tape) || (!features && !pooled)) return stlt_set_error(STLT_EINVAL, "%s: null pointer", who);
  TrunkPlan P;
  if (!trunk_plan(B, T, H, W, &P)) return stlt_set_error(STLT_EINVAL, "%s: bad video shape or too small for the trunk", who);
  if (!workspace || workspace_bytes < (size_t)P.ws.bytes)
    return stlt_set_error(STLT_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, (size_t)P.ws.bytes);
  if (train && tape_bytes < (size_t)P.tape.bytes)
    return stlt_set_error(STLT_EWORKSPACE, "%s: tape of %zu bytes, %lld needed", who, tape_bytes, (long long)P.tape.bytes);
  if (((uintptr_t)workspace & 255) || ((uintptr_t)tape & 255))
    return stlt_set_error(STLT_EINVAL, "%s: %s must be 256-byte aligned", who, train ? "workspace and tape" : "workspace");
  char* ws = (char*)workspace;
  char* tp = (char*)tape;
  auto at = [](char* base, int64_t off) { return (float*)(base + off); };
  float* xin = train ? at(tp, P.tape.xin) : at(ws, P.ws.xin);
  float* stem = train ? at(tp, P.tape.stem) : at(ws, P.ws.t1);
  float* pool = train ? at(tp, P.tape.pool) : at(ws, P.ws.x[0]);
  float* DS = at(ws, P.ws.ds);
  float* part = at(ws, P.ws.part);
  auto conv = [&](int i, const float* x, const float* res, int relu, float* y) -> int {
    const stlt_r3d_conv& c = p->conv[i];
    return launch_conv(P.g[i], x, c.w, c.bn_w, c.bn_b, c.bn_mean, c.bn_var, p->bn_eps, res, relu, y, P.fwd_splits[i], part, (hipStream_t)stream);
  };
  if (int e = stlt_ncdhw_to_ndhwc(video, B, 3, T, H, W, 4, xin, stream)) return e;
  const ConvGeom& s0 = P.g[0];
  if (int e = conv(0, xin, nullptr, 1, stem)) return e;  // stem + bn1 + relu
  if (int e = train ? stlt_maxpool3d_ndhwc_train(stem, B, s0.To, s0.Ho, s0.Wo, s0.N, pool, (uint8_t*)(tp + P.tape.argmax), stream)
                    : stlt_maxpool3d_ndhwc(stem, B, s0.To, s0.Ho, s0.Wo, s0.N, pool, stream))
    return e;
  const float* cur = pool;
  for (int b = 0; b < R3D_NBLOCKS; ++b) {
    const TrunkBlock& k = P.blk[b];
    float* a1 = train ? at(tp, k.a1) : at(ws, P.ws.t1);
    float* a2 = train ? at(tp, k.a2) : at(ws, P.ws.t2);
    float* y = train ? at(tp, k.y) : at(ws, P.ws.x[(b + 1) & 1]);
    if (int e = conv(k.conv1, cur, nullptr, 1, a1)) return e;     // conv1 + bn1 + relu
    if (int e = conv(k.conv1 + 1, a1, nullptr, 1, a2)) return e;  // conv2 + bn2 + relu (the block's stride)
    const float* shortcut = cur;
    if (k.ds) {  // 1x1x1 under the block's stride, + BN
      if (int e = conv(k.conv1 + 3, cur, nullptr, 0, DS)) return e;
      shortcut = DS;
    }
    if (int e = conv(k.conv1 + 2, a2, shortcut, 1, y)) return e;  // conv3 + bn3 + shortcut, relu
    cur = y;
  }
  const ConvGeom& last = P.g[P.blk[R3D_NBLOCKS - 1].conv1 + 2];
  const int64_t Pn = (int64_t)last.To * last.Ho * last.Wo;
  if (features)
    if (int e = stlt_ndhwc_to_ncdhw(cur, B, Pn, last.N, features, stream)) return e;
  if (pooled)
    if (int e = stlt_avgpool_ndhwc(cur, B, Pn, last.N, pooled, stream)) return e;
  return 0;
}

extern "C" {

int stlt_r3d_forward(const stlt_r3d_params* p, const float* video, int64_t B, int64_t T, int64_t H, int64_t W, void* workspace, size_t workspace_bytes,
                     float* features, float* pooled, stlt_stream_t stream) {
  return r3d_forward("stlt_r3d_forward", false, p, video, B, T, H, W, workspace, workspace_bytes, nullptr, 0, features, pooled, stream);
}

int stlt_r3d_train_forward(const stlt_r3d_params* p, const float* video, int64_t B, int64_t T, int64_t H, int64_t W, void* workspace, size_t workspace_bytes,
                           void* tape, size_t tape_bytes, float* features, float* pooled, stlt_stream_t stream) {
  return r3d_forward("stlt_r3d_train_forward", true, p, video, B, T, H, W, workspace, workspace_bytes, tape, tape_bytes, features, pooled, stream);
}

}  // extern "C"

// the trunk's reverse sweep, written once: stlt_r3d_backward (dweight, no dvideo) and stlt_r3d_backward_inputs (either or both)
// (dlayer: stlt_r3d_backward_layer's stop — the sweep ends at the first block of stage `layer` + 1, whose input gradient goes to dlayer
// without the ReLU mask of that input)
static int r3d_backward_sweep(const char* who, const stlt_r3d_params* p, const float* const* dgrad_w, const void* tape, size_t tape_bytes, int64_t B,
                              int64_t T, int64_t H, int64_t W, const float* dfeatures, const float* dpooled, float* const* dweight, int accumulate,
                              float* dvideo, void* workspace, size_t workspace_bytes, stlt_stream_t stream, int layer = 0, float* dlayer = nullptr) {
  if (int e = check_r3d_params(p, who)) return e;
  if (!dgrad_w || !tape) return stlt_set_error(STLT_EINVAL, "%s: null pointer", who);
  if ((dfeatures == nullptr) == (dpooled == nullptr)) return stlt_set_error(STLT_EINVAL, "%s: pass exactly one of dfeatures and dpooled", who);
  for (int i = 0; i < STLT_R3D_CONVS; ++i) {
    if (dweight && !dweight[i]) return stlt_set_error(STLT_EINVAL, "%s: weight gradient %d is null", who, i);
    if (i > 0 && (!dgrad_w[i] || ((uintptr_t)dgrad_w[i] & 15))) return stlt_set_error(STLT_EINVAL, "%s: dgrad copy %d is null or not 16-byte aligned", who, i);
  }
  if (dvideo && (!dgrad_w[0] || ((uintptr_t)dgrad_w[0] & 15)))
    return stlt_set_error(STLT_EINVAL, "%s: the stem's thin dgrad copy (dgrad_w[0], stlt_conv3d_repack_dgrad_thin) is null or not 16-byte aligned", who);
  TrunkPlan P;
  if (!trunk_plan(B, T, H, W, &P)) return stlt_set_error(STLT_EINVAL, "%s: bad video shape or too small for the trunk", who);
  if (tape_bytes < (size_t)P.tape.bytes) return stlt_set_error(STLT_EWORKSPACE, "%s: tape of %zu bytes, %lld needed", who, tape_bytes, (long long)P.tape.bytes);
  if (!workspace || workspace_bytes < (size_t)P.bws.bytes)
    return stlt_set_error(STLT_EWORKSPACE, "%s: workspace of %zu bytes, %lld needed", who, workspace_bytes, (long long)P.bws.bytes);
  if (((uintptr_t)workspace & 255) || ((uintptr_t)tape & 255)) return stlt_set_error(STLT_EINVAL, "%s: workspace and tape must be 256-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  auto taped = [&](int64_t off) { return (const float*)((const char*)tape + off); };
  auto work = [&](int64_t off) { return (float*)((char*)workspace + off); };
  float* G3 = work(P.bws.g3);  // masked pre-ReLU gradient at the block's output
  float* G2 = work(P.bws.g2);
  float* G1 = work(P.bws.g1);
  float* GX = work(P.bws.gx);  // ... at its input (the block before's G3)
  float* GS = work(P.bws.gs);  // at the stem's output
  float* part = work(P.bws.part);
  const float eps = p->bn_eps;
  const int stop = dlayer ? stage_first_block(P, layer + 1) : -1;  // the last block the sweep visits
  auto wgrad = [&](int i, const float* x, const float* g) -> int {
    if (!dweight) return 0;  // the input-only sweep: no weight-gradient product
    const ConvGeom& c = P.g[i];
    const int cin_w = i == 0 ? 3 : c.C;
    return launch_wgrad(c, x, g, cin_w, nullptr, p->conv[i].bn_w, p->conv[i].bn_var, eps, accumulate, dweight[i], wgrad_plan_splits(c), part, s);
  };
  auto dgrad = [&](int i, const float* g, const float* mask, const float* add, float* dx) {
    return launch_dgrad(P.g[i], g, dgrad_w[i], nullptr, mask, add, dx, part, P.bwd_part_bytes, 0, s, add == dx);
  };
  {
    const TrunkBlock& top = P.blk[R3D_NBLOCKS - 1];
    const ConvGeom& last = P.g[top.conv1 + 2];
    const int64_t Pn = (int64_t)last.To * last.Ho * last.Wo;
    const int64_t n = B * Pn * last.N;
    hipLaunchKernelGGL(r3d_grad_in_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, dpooled, dfeatures, taped(top.y), B, (int)Pn, last.N, G3);
    if (int e = stlt_check_launch("r3d_grad_in_kernel")) return e;
  }
  for (int bi = R3D_NBLOCKS - 1; bi >= 0; --bi) {
    const TrunkBlock& k = P.blk[bi];
    const int ci = k.conv1;
    const float *a1 = taped(k.a1), *a2 = taped(k.a2), *x = taped(k.x);
    const float* xmask = bi > 0 ? x : nullptr;  // the first block reads the max-pool output, which has no ReLU after it
    if (int e = wgrad(ci + 2, a2, G3)) return e;
    if (int e = dgrad(ci + 2, G3, a2, nullptr, G2)) return e;
    if (int e = wgrad(ci + 1, a1, G2)) return e;
    if (int e = dgrad(ci + 1, G2, a1, nullptr, G1)) return e;
    if (int e = wgrad(ci, x, G1)) return e;
    if (bi == stop) {  // the same two products into dlayer, unmasked: the gradient at the stage's output after its ReLU, as a hook there sees it
      if (int e = dgrad(ci, G1, nullptr, k.ds ? nullptr : G3, dlayer)) return e;
      return k.ds ? dgrad(ci + 3, G3, nullptr, dlayer, dlayer) : 0;
    }
    // block input: conv1's data gradient + the shortcut's (identity: G3 itself), masked by the input's ReLU
    if (int e = dgrad(ci, G1, xmask, k.ds ? nullptr : G3, GX)) return e;
    if (k.ds) {
      if (int e = wgrad(ci + 3, x, G3)) return e;
      if (int e = dgrad(ci + 3, G3, xmask, GX, GX)) return e;
    }
    std::swap(G3, GX);
  }
  // G3 now holds the gradient at the max-pool output: max-pool backward with the stem's ReLU mask, then the stem's weight gradient
  const ConvGeom& s0 = P.g[0];
  if (int e = stlt_maxpool3d_ndhwc_bwd(G3, (const uint8_t*)taped(P.tape.argmax), B, s0.To, s0.Ho, s0.Wo, s0.N, taped(P.tape.stem), GS, stream)) return e;
  if (int e = wgrad(0, taped(P.tape.xin), GS)) return e;
  if (!dvideo) return 0;
  // the stem's data gradient, straight into video_frames' layout (the BN scale is folded into the thin copy)
  const ThinGeom tg{(int)B, (int)T, (int)H, (int)W, s0.To, s0.Ho, s0.Wo, s0.N, 3, (int)cdiv(s0.Ho, TH_TI), (int)cdiv(s0.Wo, TH_TJ)};
  return launch_dgrad_thin(tg, GS, dgrad_w[0], dvideo, 1, s);
}

extern "C" {

int stlt_r3d_backward(const stlt_r3d_params* p, const float* const* dgrad_w, const void* tape, size_t tape_bytes, int64_t B, int64_t T, int64_t H, int64_t W,
                      const float* dfeatures, const float* dpooled, float* const* dweight, int accumulate, void* workspace, size_t workspace_bytes,
                      stlt_stream_t stream) {
  if (!dweight) {  // this entry point always writes the weight gradients
    if (int e = check_r3d_params(p, "stlt_r3d_backward")) return e;
    return stlt_set_error(STLT_EINVAL, "stlt_r3d_backward: null pointer");
  }
  return r3d_backward_sweep("stlt_r3d_backward", p, dgrad_w, tape, tape_bytes, B, T, H, W, dfeatures, dpooled, dweight, accumulate, nullptr, workspace,
                            workspace_bytes, stream);
}

int stlt_r3d_backward_inputs(const stlt_r3d_params* p, const float* const* dgrad_w, const void* tape, size_t tape_bytes, int64_t B, int64_t T, int64_t H,
                             int64_t W, const float* dfeatures, const float* dpooled, float* const* dweight, int accumulate, float* dvideo,
                             void* workspace, size_t workspace_bytes, stlt_stream_t stream) {
  if (!dweight && !dvideo) return stlt_set_error(STLT_EINVAL, "stlt_r3d_backward_inputs: dweight and dvideo are both null: nothing to compute");
  return r3d_backward_sweep("stlt_r3d_backward_inputs", p, dgrad_w, tape, tape_bytes, B, T, H, W, dfeatures, dpooled, dweight, accumulate, dvideo, workspace,
                            workspace_bytes, stream);
}

int stlt_r3d_layer_geometry(int64_t B, int64_t T, int64_t H, int64_t W, int layer, int64_t* dims, size_t* tape_offset) {
  if (layer < 1 || layer > R3D_LAYERS) return stlt_set_error(STLT_EINVAL, "stlt_r3d_layer_geometry: layer is 1 to %d, got %d", R3D_LAYERS, layer);
  if (!dims || !tape_offset) return stlt_set_error(STLT_EINVAL, "stlt_r3d_layer_geometry: null pointer");
  TrunkPlan P;
  if (!trunk_plan(B, T, H, W, &P)) return stlt_set_error(STLT_EINVAL, "stlt_r3d_layer_geometry: bad video shape or too small for the trunk");
  const TrunkBlock& k = P.blk[stage_first_block(P, layer + 1) - 1];  // the stage's last block
  const ConvGeom& g = P.g[k.conv1 + 2];
  dims[0] = g.To; dims[1] = g.Ho; dims[2] = g.Wo; dims[3] = g.N;
  *tape_offset = (size_t)k.y;
  return 0;
}

int stlt_r3d_backward_layer(const stlt_r3d_params* p, const float* const* dgrad_w, const void* tape, size_t tape_bytes, int64_t B, int64_t T, int64_t H,
                            int64_t W, const float* dfeatures, const float* dpooled, int layer, float* dlayer, void* workspace, size_t workspace_bytes,
                            stlt_stream_t stream) {
  if (layer < 1 || layer >= R3D_LAYERS)
    return stlt_set_error(STLT_EINVAL, "stlt_r3d_backward_layer: layer is 1 to %d (the last stage's gradient is the call's own input), got %d", R3D_LAYERS - 1, layer);
  if (!dlayer || ((uintptr_t)dlayer & 15)) return stlt_set_error(STLT_EINVAL, "stlt_r3d_backward_layer: dlayer is null or not 16-byte aligned");
  return r3d_backward_sweep("stlt_r3d_backward_layer", p, dgrad_w, tape, tape_bytes, B, T, H, W, dfeatures, dpooled, nullptr, 0, nullptr, workspace,
                            workspace_bytes, stream, layer, dlayer);
}

size_t stlt_conv3d_repack_dgrad_thin_floats(const stlt_conv3d_desc* d) {
  if (check_thin_desc(d, "stlt_conv3d_repack_dgrad_thin_floats", nullptr)) return 0;
  return (size_t)(1792 * d->c_out);
}

int stlt_conv3d_repack_dgrad_thin(const float* w, const stlt_conv3d_desc* d, const float* scale, float* out, stlt_stream_t stream) {
  ThinGeom g;
  if (int e = check_thin_desc(d, "stlt_conv3d_repack_dgrad_thin", &g)) return e;
  if (!w || !out) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_repack_dgrad_thin: null pointer");
  const int64_t n = 1792 * (int64_t)g.N;
  hipLaunchKernelGGL(conv3d_repack_dgrad_thin_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, 256), 4096)), dim3(256), 0, (hipStream_t)stream, w, g.N, g.c_in,
                     scale, out);
  return stlt_check_launch("conv3d_repack_dgrad_thin_kernel");
}

int stlt_conv3d_bwd_data_thin(const stlt_conv3d_desc* d, const float* dy, const float* w_dgrad_thin, float* dx, int dx_layout, stlt_stream_t stream) {
  ThinGeom g;
  if (int e = check_thin_desc(d, "stlt_conv3d_bwd_data_thin", &g)) return e;
  if (!dy || !w_dgrad_thin || !dx) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data_thin: null pointer");
  if (dx_layout != STLT_DX_NDHWC && dx_layout != STLT_DX_NCDHW)
    return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data_thin: dx_layout must be STLT_DX_NDHWC or STLT_DX_NCDHW, got %d", dx_layout);
  if (((uintptr_t)dy & 15) || ((uintptr_t)w_dgrad_thin & 15))
    return stlt_set_error(STLT_EINVAL, "stlt_conv3d_bwd_data_thin: dy and w_dgrad_thin must be 16-byte aligned");
  return launch_dgrad_thin(g, dy, w_dgrad_thin, dx, dx_layout == STLT_DX_NCDHW, (hipStream_t)stream);
}

}  // extern "C"
