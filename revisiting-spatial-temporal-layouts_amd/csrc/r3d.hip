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
template <int BN>
__global__ __launch_bounds__(256) void conv3d_igemm_kernel(const float* __restrict__ x, const float* __restrict__ w, ConvGeom g,
                                                           const float* __restrict__ bn_w, const float* __restrict__ bn_b,
                                                           const float* __restrict__ bn_mean, const float* __restrict__ bn_var, float eps,
                                                           const float* __restrict__ res, int relu, float* __restrict__ y, int slabs_per_split) {
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
    if (!split) bn_coeffs(bn_w, bn_b, bn_mean, bn_var, eps, gn, &sc, &sh);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int gm = m0 + wm + 16 * i + 4 * lg + q;
        if (gm >= g.M) continue;
        const int64_t o = (int64_t)gm * g.N + gn;
        if (split) { y[o] = acc[i][j][q]; continue; }
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

// number of contraction splits for an (M, N, K) conv launch (1: whole tiles, no workspace)
int64_t conv_plan_splits(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = cdiv(M, BM) * cdiv(N, conv_bn_tile(N));
  const int64_t slabs = cdiv(K, CK);
  if (tiles >= SPLIT_TARGET_WG / 2) return 1;
  int64_t splits = cdiv(SPLIT_TARGET_WG, tiles);
  if (splits > slabs / SPLIT_MIN_SLABS) splits = slabs / SPLIT_MIN_SLABS;
  if (splits > SPLIT_MAX) splits = SPLIT_MAX;
  if (splits < 2) return 1;
  const int64_t per = cdiv(slabs, splits);
  return cdiv(slabs, per);
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
  const int64_t M = d->B * To * Ho * Wo, K = d->kt * d->kh * d->kw * d->c_in;
  if (M > 0x7fffff00LL || K > 0x7fffff00LL || d->B * d->T * d->H * d->W > 0x7fffff00LL || M * d->c_out > (1LL << 40))
    return stlt_set_error(STLT_EINVAL, "conv3d: shape too large");
  if (cdiv(M, BM) > 0x7fffffffLL || cdiv(d->c_out, 64) > 65535) return stlt_set_error(STLT_EINVAL, "conv3d: too many output tiles");
  *g = ConvGeom{(int)d->B, (int)d->T, (int)d->H, (int)d->W, (int)d->c_in, (int)To, (int)Ho, (int)Wo, (int)d->c_out, (int)d->kt, (int)d->kh, (int)d->kw,
                (int)d->st, (int)d->sh, (int)d->sw, (int)d->pt, (int)d->ph, (int)d->pw, (int)M, (int)K};
  return 0;
}

int64_t conv_split_bytes(const ConvGeom& g, int64_t splits) { return splits > 1 ? splits * (int64_t)g.M * g.N * (int64_t)sizeof(float) : 0; }

int launch_conv(const ConvGeom& g, const float* x, const float* w, const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var,
                float eps, const float* res, int relu, float* y, int64_t splits, float* part, hipStream_t s) {
  const int bn = conv_bn_tile(g.N);
  const int64_t slabs = cdiv(g.K, CK);
  if (splits > slabs) splits = slabs;
  const int64_t per = cdiv(slabs, splits);
  splits = cdiv(slabs, per);
  const dim3 grid((unsigned)cdiv(g.M, BM), (unsigned)cdiv(g.N, bn), (unsigned)splits), block(256);
  float* dst = splits > 1 ? part : y;
  if (bn == 64)
    hipLaunchKernelGGL(conv3d_igemm_kernel<64>, grid, block, 0, s, x, w, g, bn_w, bn_b, bn_mean, bn_var, eps, res, relu, dst, (int)per);
  else
    hipLaunchKernelGGL(conv3d_igemm_kernel<128>, grid, block, 0, s, x, w, g, bn_w, bn_b, bn_mean, bn_var, eps, res, relu, dst, (int)per);
  if (int e = stlt_check_launch("conv3d_igemm_kernel")) return e;
  if (splits > 1) {
    hipLaunchKernelGGL(conv3d_split_finish_kernel, dim3((unsigned)cdiv((int64_t)g.M * g.N, 256)), dim3(256), 0, s, part, (int)splits, g.M, g.N, bn_w, bn_b,
                       bn_mean, bn_var, eps, res, relu, y);
    return stlt_check_launch("conv3d_split_finish_kernel");
  }
  return 0;
}

// ---- the trunk's plan: the 53 convolutions in state-dict order (stem; per block conv1, conv2, conv3, [downsample]) ----
constexpr int R3D_BLOCKS[4] = {3, 4, 6, 3};
constexpr int R3D_PLANES[4] = {64, 128, 256, 512};

struct TrunkDims {
  int64_t act_elems = 0;    // largest block-level activation (per buffer)
  int64_t stem_elems = 0;   // stem output
  int64_t part_bytes = 0;   // largest split-K partial buffer
  int64_t To = 0, Ho = 0, Wo = 0;
  bool ok = false;
};

// walk the trunk's shapes (no launches): the workspace plan of stlt_r3d_workspace_bytes and stlt_r3d_forward
TrunkDims trunk_dims(int64_t B, int64_t T, int64_t H, int64_t W) {
  TrunkDims d;
  auto conv = [&](int64_t& t, int64_t& h, int64_t& w, int64_t cin, int64_t cout, int k, int s, int p, int st_t) {
    const int64_t to = out_dim(t, k, st_t, p), ho = out_dim(h, k, s, p), wo = out_dim(w, k, s, p);
    const int64_t M = B * to * ho * wo, K = (int64_t)k * k * k * cin;
    const int64_t sp = conv_plan_splits(M, cout, K);
    if (sp > 1) d.part_bytes = std::max<int64_t>(d.part_bytes, sp * M * cout * (int64_t)sizeof(float));
    t = to; h = ho; w = wo;
    return M * cout;
  };
  int64_t t = T, h = H, w = W;
  // stem: 7x7x7, stride (1, 2, 2), pad 3 — 3 (padded to 4) -> 64
  {
    const int64_t to = out_dim(t, 7, 1, 3), ho = out_dim(h, 7, 2, 3), wo = out_dim(w, 7, 2, 3);
    if (to <= 0 || ho <= 0 || wo <= 0) return d;
    const int64_t M = B * to * ho * wo, sp = conv_plan_splits(M, 64, 343 * 4);
    if (sp > 1) d.part_bytes = std::max<int64_t>(d.part_bytes, sp * M * 64 * (int64_t)sizeof(float));
    d.stem_elems = M * 64;
    t = to; h = ho; w = wo;
  }
  t = out_dim(t, 3, 2, 1); h = out_dim(h, 3, 2, 1); w = out_dim(w, 3, 2, 1);  // max-pool
  int64_t cin = 64;
  d.act_elems = B * t * h * w * cin;
  for (int L = 0; L < 4; ++L) {
    const int64_t planes = R3D_PLANES[L];
    for (int blk = 0; blk < R3D_BLOCKS[L]; ++blk) {
      const int s = (L > 0 && blk == 0) ? 2 : 1;
      int64_t t1 = t, h1 = h, w1 = w;
      d.act_elems = std::max(d.act_elems, conv(t1, h1, w1, cin, planes, 1, 1, 0, 1));
      d.act_elems = std::max(d.act_elems, conv(t1, h1, w1, planes, planes, 3, s, 1, s));
      d.act_elems = std::max(d.act_elems, conv(t1, h1, w1, planes, planes * 4, 1, 1, 0, 1));
      if (blk == 0) {
        int64_t t2 = t, h2 = h, w2 = w;
        conv(t2, h2, w2, cin, planes * 4, 1, s, 0, s);
      }
      t = t1; h = h1; w = w1;
      cin = planes * 4;
    }
  }
  d.To = t; d.Ho = h; d.Wo = w;
  d.ok = true;
  return d;
}

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

}  // namespace

extern "C" {

size_t stlt_conv3d_workspace_bytes(const stlt_conv3d_desc* d, int n_split) {
  ConvGeom g;
  if (check_desc(d, &g)) return 0;
  const int64_t splits = n_split <= 0 ? conv_plan_splits(g.M, g.N, g.K) : n_split;
  return (size_t)conv_split_bytes(g, splits);
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
  int64_t splits = n_split == 0 ? conv_plan_splits(g.M, g.N, g.K) : n_split;
  if (n_split == 0 && (!workspace || workspace_bytes < (size_t)conv_split_bytes(g, splits))) splits = 1;  // automatic: split only into lent workspace
  if (splits > 1 && (!workspace || workspace_bytes < (size_t)conv_split_bytes(g, splits)))
    return stlt_set_error(STLT_EWORKSPACE, "stlt_conv3d_fwd: %lld splits need %lld workspace bytes, %zu lent", (long long)splits,
                          (long long)conv_split_bytes(g, splits), workspace_bytes);
  return launch_conv(g, x, w, bn_w, bn_b, bn_mean, bn_var, bn_eps, residual, relu, y, splits, (float*)workspace, (hipStream_t)stream);
}

int stlt_conv3d_repack(const float* w, int64_t c_out, int64_t c_in, int64_t kt, int64_t kh, int64_t kw, int64_t c_pad, float* out, stlt_stream_t stream) {
  if (!w || !out) return stlt_set_error(STLT_EINVAL, "stlt_conv3d_repack: null pointer");
  if (c_out <= 0 || c_in <= 0 || kt <= 0 || kh <= 0 || kw <= 0 || c_pad < c_in || c_pad > (1 << 20) || kt * kh * kw > (1 << 20) || c_out > (1 << 24))
    return stlt_set_error(STLT_EINVAL, "stlt_conv3d_repack: bad shape");
  const int64_t n = c_out * kt * kh * kw * c_pad;
  hipLaunchKernelGGL(conv3d_repack_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w, c_out, (int)c_in, (int)(kt * kh * kw),
                     (int)c_pad, out);
  return stlt_check_launch("conv3d_repack_kernel");
}

int stlt_ncdhw_to_ndhwc(const float* x, int64_t B, int64_t C, int64_t T, int64_t H, int64_t W, int64_t c_pad, float* y, stlt_stream_t stream) {
  if (!x || !y) return stlt_set_error(STLT_EINVAL, "stlt_ncdhw_to_ndhwc: null pointer");
  if (B < 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || c_pad < C || c_pad > (1 << 20) || B * T * H * W * c_pad > (1LL << 40))
    return stlt_set_error(STLT_EINVAL, "stlt_ncdhw_to_ndhwc: bad shape");
  const int64_t n = B * T * H * W * c_pad;
  if (n == 0) return 0;
  hipLaunchKernelGGL(ncdhw_to_ndhwc_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, B, (int)C, T * H * W, (int)c_pad, y);
  return stlt_check_launch("ncdhw_to_ndhwc_kernel");
}

int stlt_ndhwc_to_ncdhw(const float* x, int64_t B, int64_t P, int64_t C, float* y, stlt_stream_t stream) {
  if (!x || !y) return stlt_set_error(STLT_EINVAL, "stlt_ndhwc_to_ncdhw: null pointer");
  if (B < 0 || P <= 0 || C <= 0 || C > (1 << 24) || B * P * C > (1LL << 40)) return stlt_set_error(STLT_EINVAL, "stlt_ndhwc_to_ncdhw: bad shape");
  const int64_t n = B * P * C;
  if (n == 0) return 0;
  hipLaunchKernelGGL(ndhwc_to_ncdhw_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, B, P, (int)C, y);
  return stlt_check_launch("ndhwc_to_ncdhw_kernel");
}

int stlt_maxpool3d_ndhwc(const float* x, int64_t B, int64_t T, int64_t H, int64_t W, int64_t C, float* y, stlt_stream_t stream) {
  if (!x || !y) return stlt_set_error(STLT_EINVAL, "stlt_maxpool3d_ndhwc: null pointer");
  if (B < 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || T > (1 << 24) || H > (1 << 24) || W > (1 << 24) || C > (1 << 24) || B * T * H * W * C > (1LL << 40))
    return stlt_set_error(STLT_EINVAL, "stlt_maxpool3d_ndhwc: bad shape");
  const int64_t To = out_dim(T, 3, 2, 1), Ho = out_dim(H, 3, 2, 1), Wo = out_dim(W, 3, 2, 1);
  const int64_t n = B * To * Ho * Wo * C;
  if (n == 0) return 0;
  hipLaunchKernelGGL(maxpool3d_ndhwc_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, (int)B, (int)T, (int)H, (int)W, (int)C,
                     (int)To, (int)Ho, (int)Wo, y);
  return stlt_check_launch("maxpool3d_ndhwc_kernel");
}

int stlt_avgpool_ndhwc(const float* x, int64_t B, int64_t P, int64_t C, float* y, stlt_stream_t stream) {
  if (!x || !y) return stlt_set_error(STLT_EINVAL, "stlt_avgpool_ndhwc: null pointer");
  if (B < 0 || P <= 0 || C <= 0 || P > (1 << 24) || C > (1 << 24) || B * P * C > (1LL << 40)) return stlt_set_error(STLT_EINVAL, "stlt_avgpool_ndhwc: bad shape");
  if (B == 0) return 0;
  hipLaunchKernelGGL(avgpool_ndhwc_kernel, dim3((unsigned)cdiv(B * C, 256)), dim3(256), 0, (hipStream_t)stream, x, B, (int)P, (int)C, y);
  return stlt_check_launch("avgpool_ndhwc_kernel");
}

size_t stlt_r3d_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W) {
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || T > 4096 || H > 4096 || W > 4096 || B > (1 << 20)) return 0;
  const TrunkDims d = trunk_dims(B, T, H, W);
  if (!d.ok) return 0;
  const int64_t f = sizeof(float);
  return (size_t)(align256(B * T * H * W * 4 * f) + 3 * align256(d.act_elems * f) + align256(std::max(d.stem_elems, 2 * d.act_elems) * f) +
                  align256(d.part_bytes));
}

int stlt_r3d_forward(const stlt_r3d_params* p, const float* video, int64_t B, int64_t T, int64_t H, int64_t W, void* workspace, size_t workspace_bytes,
                     float* features, float* pooled, stlt_stream_t stream) {
  if (!p || !video || (!features && !pooled)) return stlt_set_error(STLT_EINVAL, "stlt_r3d_forward: null pointer");
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || T > 4096 || H > 4096 || W > 4096 || B > (1 << 20)) return stlt_set_error(STLT_EINVAL, "stlt_r3d_forward: bad video shape");
  for (int i = 0; i < STLT_R3D_CONVS; ++i) {
    const stlt_r3d_conv& c = p->conv[i];
    if (!c.w || !c.bn_w || !c.bn_b || !c.bn_mean || !c.bn_var) return stlt_set_error(STLT_EINVAL, "stlt_r3d_forward: conv %d has a null weight or BatchNorm buffer", i);
    if ((uintptr_t)c.w & 15) return stlt_set_error(STLT_EINVAL, "stlt_r3d_forward: packed weight %d is not 16-byte aligned", i);
  }
  const TrunkDims d = trunk_dims(B, T, H, W);
  if (!d.ok || d.To <= 0 || d.Ho <= 0 || d.Wo <= 0) return stlt_set_error(STLT_EINVAL, "stlt_r3d_forward: video too small for the trunk");
  const size_t need = stlt_r3d_workspace_bytes(B, T, H, W);
  if (!workspace || workspace_bytes < need)
    return stlt_set_error(STLT_EWORKSPACE, "stlt_r3d_forward: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  if ((uintptr_t)workspace & 255) return stlt_set_error(STLT_EINVAL, "stlt_r3d_forward: workspace must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t f = sizeof(float);
  char* base = (char*)workspace;
  float* xin = (float*)base; base += align256(B * T * H * W * 4 * f);
  float* X0 = (float*)base; base += align256(d.act_elems * f);
  float* X1 = (float*)base; base += align256(d.act_elems * f);
  float* DS = (float*)base; base += align256(d.act_elems * f);
  float* T1 = (float*)base;
  float* T2 = T1 + d.act_elems;
  base += align256(std::max(d.stem_elems, 2 * d.act_elems) * f);
  float* part = (float*)base;
  const float eps = p->bn_eps;

  if (int e = stlt_ncdhw_to_ndhwc(video, B, 3, T, H, W, 4, xin, stream)) return e;
  int ci = 0;
  // conv helper: x (B, t, h, w, cin) -> y; t/h/w updated to the output's
  auto conv = [&](const float* x, int64_t& t, int64_t& h, int64_t& w, int64_t cin, int64_t cout, int k, int sp, int st_t, int pad, const float* res, int relu,
                  float* y) -> int {
    const stlt_conv3d_desc desc{B, t, h, w, cin, cout, k, k, k, st_t, sp, sp, pad, pad, pad};
    ConvGeom g;
    if (int e = check_desc(&desc, &g)) return e;
    const stlt_r3d_conv& c = p->conv[ci++];
    const int64_t splits = conv_plan_splits(g.M, g.N, g.K);
    if (int e = launch_conv(g, x, c.w, c.bn_w, c.bn_b, c.bn_mean, c.bn_var, eps, res, relu, y, splits, part, s)) return e;
    t = g.To; h = g.Ho; w = g.Wo;
    return 0;
  };
  int64_t t = T, h = H, w = W;
  // stem (7x7x7, stride (1,2,2), pad 3) + bn1 + relu, then the max-pool
  if (int e = conv(xin, t, h, w, 4, 64, 7, 2, 1, 3, nullptr, 1, T1)) return e;
  if (int e = stlt_maxpool3d_ndhwc(T1, B, t, h, w, 64, X0, stream)) return e;
  t = out_dim(t, 3, 2, 1); h = out_dim(h, 3, 2, 1); w = out_dim(w, 3, 2, 1);
  int64_t cin = 64;
  float *cur = X0, *nxt = X1;
  for (int L = 0; L < 4; ++L) {
    const int64_t planes = R3D_PLANES[L];
    for (int blk = 0; blk < R3D_BLOCKS[L]; ++blk) {
      const int sp = (L > 0 && blk == 0) ? 2 : 1;
      int64_t t1 = t, h1 = h, w1 = w;
      if (int e = conv(cur, t1, h1, w1, cin, planes, 1, 1, 1, 0, nullptr, 1, T1)) return e;              // conv1 + bn1 + relu
      if (int e = conv(T1, t1, h1, w1, planes, planes, 3, sp, sp, 1, nullptr, 1, T2)) return e;          // conv2 + bn2 + relu (stride)
      // conv3 + bn3 (+ shortcut) + relu; the downsample (1x1x1, stride, + BN) comes after conv3 in state-dict order
      const int c3 = ci;
      const float* shortcut = cur;
      if (blk == 0) {
        ci = c3 + 1;
        int64_t t2 = t, h2 = h, w2 = w;
        if (int e = conv(cur, t2, h2, w2, cin, planes * 4, 1, sp, sp, 0, nullptr, 0, DS)) return e;
        shortcut = DS;
        ci = c3;
      }
      if (int e = conv(T2, t1, h1, w1, planes, planes * 4, 1, 1, 1, 0, shortcut, 1, nxt)) return e;
      if (blk == 0) ci = c3 + 2;
      t = t1; h = h1; w = w1;
      cin = planes * 4;
      std::swap(cur, nxt);
    }
  }
  if (ci != STLT_R3D_CONVS) return stlt_set_error(STLT_EINVAL, "stlt_r3d_forward: internal plan error (%d convs)", ci);
  const int64_t P = t * h * w;
  if (features)
    if (int e = stlt_ndhwc_to_ncdhw(cur, B, P, cin, features, stream)) return e;
  if (pooled)
    if (int e = stlt_avgpool_ndhwc(cur, B, P, cin, pooled, stream)) return e;
  return 0;
}

}  // extern "C"
