// Grad-CAM (Selvaraju et al., ICCV 2017) and HiResCAM (Draelos and Carin, 2020) on the device: a class activation map at a stage of the
// R3D-50 trunk is the channel sum of the stage's activations a, weighted by the gradient g of one logit with respect to them — by its
// mean over the positions (Grad-CAM: alpha[b,c] = mean_p g[b,p,c], cam[b,p] = relu(sum_c alpha[b,c] a[b,p,c])) or element by element
// (HiResCAM: cam[b,p] = relu(sum_c g[b,p,c] a[b,p,c])).  The activations and the gradient exist (r3d.hip: the tape, the reverse sweep
// stopped at a stage); this file holds the two reductions that turn them into a map and the trilinear resize that lays a map over the video.
//
//   cam_weights_ndhwc_kernel   g (B,P,C): lanes along c (a float4 of channels per lane when VEC), a wave per chunk of CAM_CHUNK positions,
//                              added in order by four accumulators; one chunk: alpha directly, more: partials into scratch, then
//   cam_weights_finish_kernel  the partials of a (b,c) added in ascending chunk order, divided by P.
//   cam_weights_ncdhw_kernel   g (B,C,P): a wave per (b,c) row, lane l adds elements l, l + 64, ... in order, then the DPP wave sum.
//   cam_map_ndhwc_kernel       a (B,P,C): a wave per position, lanes along c, fmaf chain per lane, then the DPP wave sum.
//   cam_map_ncdhw_kernel       a (B,C,P): a workgroup per CAM_PT positions of a clip, CAM_CG lane groups along c, each lane an fmaf chain over
//                              c = group, group + CAM_CG, ...; the groups' partials added in ascending order through LDS.
//   cam_upsample_kernel        one thread per output element of the trilinear resize.
//
// Every sum has one owner and one order, which depends on the shape alone: no atomics, the same bits for a clip whatever the batch.
#include "common.h"
#include "wave_dpp.h"

namespace {

constexpr int CAM_THREADS = 256;
constexpr int CAM_CHUNK = STLT_CAM_CHUNK;  // positions of one partial of the NDHWC weights: the partition of P is [0,32), [32,64), ...
constexpr int CAM_PT = 32;      // positions of one workgroup of the NCDHW map (a 128-byte line of every channel row)
constexpr int CAM_CG = 16;      // ... and its lane groups along c
constexpr int64_t CAM_MAX = 0x7fffffff;

// VEC: a lane owns channels [4 col, 4 col + 4) (16-byte loads), else channel col.  Wave w of workgroup (x, y, b) owns chunk 4 y + w and
// columns [64 x, 64 x + 64).  out: alpha (B,C) when the partition has one chunk (divided here), else scratch (B, chunks, C).
template <bool VEC>
__global__ __launch_bounds__(CAM_THREADS) void cam_weights_ndhwc_kernel(const float* __restrict__ g, int P, int C, int cols, int chunks, float* __restrict__ out) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int chunk = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int64_t b = blockIdx.z;
  if (col >= cols || chunk >= chunks) return;
  const int p0 = chunk * CAM_CHUNK;
  const int p1 = p0 + CAM_CHUNK < P ? p0 + CAM_CHUNK : P;
  const float* row = g + (b * P + p0) * C;
  if constexpr (VEC) {
    float4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    int p = p0;
    for (; p + 4 <= p1; p += 4, row += 4 * (int64_t)C) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(row + (int64_t)i * C + 4 * col);
        acc[i].x += v.x; acc[i].y += v.y; acc[i].z += v.z; acc[i].w += v.w;
      }
    }
    for (int i = 0; p < p1; ++p, ++i, row += C) {  // the tail goes to accumulators 0, 1, 2 in turn, as the body would have sent it
      const float4 v = *reinterpret_cast<const float4*>(row + 4 * col);
      if (i == 0) { acc[0].x += v.x; acc[0].y += v.y; acc[0].z += v.z; acc[0].w += v.w; }
      else if (i == 1) { acc[1].x += v.x; acc[1].y += v.y; acc[1].z += v.z; acc[1].w += v.w; }
      else { acc[2].x += v.x; acc[2].y += v.y; acc[2].z += v.z; acc[2].w += v.w; }
    }
    float4 s;
    s.x = (acc[0].x + acc[1].x) + (acc[2].x + acc[3].x);
    s.y = (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y);
    s.z = (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z);
    s.w = (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w);
    if (chunks == 1) {
      const float d = (float)P;
      s.x /= d; s.y /= d; s.z /= d; s.w /= d;
    }
    *reinterpret_cast<float4*>(out + (b * chunks + chunk) * C + 4 * col) = s;
  } else {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int p = p0;
    for (; p + 4 <= p1; p += 4, row += 4 * (int64_t)C) {
      a0 += row[col];
      a1 += row[(int64_t)C + col];
      a2 += row[2 * (int64_t)C + col];
      a3 += row[3 * (int64_t)C + col];
    }
    for (int i = 0; p < p1; ++p, ++i, row += C) {
      const float v = row[col];
      if (i == 0) a0 += v;
      else if (i == 1) a1 += v;
      else a2 += v;
    }
    float s = (a0 + a1) + (a2 + a3);
    if (chunks == 1) s /= (float)P;
    out[(b * chunks + chunk) * C + col] = s;
  }
}

__global__ __launch_bounds__(CAM_THREADS) void cam_weights_finish_kernel(const float* __restrict__ part, int64_t B, int P, int C, int chunks, float* __restrict__ alpha) {
  const int64_t idx = (int64_t)blockIdx.x * CAM_THREADS + threadIdx.x;
  if (idx >= B * C) return;
  const int64_t b = idx / C;
  const int c = (int)(idx - b * C);
  const float* q = part + b * chunks * C + c;
  float s = 0.f;
  for (int k = 0; k < chunks; ++k) s += q[(int64_t)k * C];
  alpha[idx] = s / (float)P;
}

// rows = B * C rows of P floats; every lane of a live wave stays active to the end (the DPP sum reads all 64)
__global__ __launch_bounds__(CAM_THREADS) void cam_weights_ncdhw_kernel(const float* __restrict__ g, int64_t rows, int P, float* __restrict__ alpha) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const float* q = g + r * P;
  float s = 0.f;
  for (int p = lane; p < P; p += 64) s += q[p];
  s = wave_sum_dpp(s);
  if (lane == 0) alpha[r] = s / (float)P;
}

// a wave per position (b,p): lane l takes the channel quads l, l + 64, ... (one 16-byte load each when VEC).  PER: w has a's shape, else w is alpha (B,C).
template <bool VEC, bool PER>
__global__ __launch_bounds__(CAM_THREADS) void cam_map_ndhwc_kernel(const float* __restrict__ a, const float* __restrict__ w, int64_t positions, int P, int C,
                                                                    int relu, float* __restrict__ cam) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= positions) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const float* ar = a + r * C;
  const float* wr = PER ? w + r * C : w + (r / P) * C;
  float s = 0.f;
  if constexpr (VEC) {
    for (int c = 4 * lane; c < C; c += 256) {
      const float4 x = *reinterpret_cast<const float4*>(ar + c);
      const float4 y = *reinterpret_cast<const float4*>(wr + c);
      s = fmaf(y.x, x.x, s);
      s = fmaf(y.y, x.y, s);
      s = fmaf(y.z, x.z, s);
      s = fmaf(y.w, x.w, s);
    }
  } else {
    for (int c = 4 * lane; c < C; c += 256) {  // the same channels in the same order, one float per load
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j < C) s = fmaf(wr[c + j], ar[c + j], s);
    }
  }
  s = wave_sum_dpp(s);
  if (lane == 0) cam[r] = (relu && !(s > 0.f)) ? 0.f : s;
}

// workgroup (tile, b): thread t = group * CAM_PT + position; group gq adds channels gq, gq + CAM_CG, ... of its position in order
template <bool PER>
__global__ __launch_bounds__(CAM_PT * CAM_CG) void cam_map_ncdhw_kernel(const float* __restrict__ a, const float* __restrict__ w, int P, int C, int relu,
                                                                        float* __restrict__ cam) {
  __shared__ float part[CAM_CG][CAM_PT];
  const int pl = threadIdx.x % CAM_PT, gq = threadIdx.x / CAM_PT;
  const int p = blockIdx.x * CAM_PT + pl;
  const int64_t b = blockIdx.y;
  float s = 0.f;
  if (p < P) {
    const float* ab = a + b * C * P + p;
    const float* wb = PER ? w + b * C * P + p : w + b * C;
#pragma unroll 4
    for (int c = gq; c < C; c += CAM_CG) s = fmaf(PER ? wb[(int64_t)c * P] : wb[c], ab[(int64_t)c * P], s);
  }
  part[gq][pl] = s;
  __syncthreads();
  if (gq == 0 && p < P) {
    float t = part[0][pl];
#pragma unroll
    for (int k = 1; k < CAM_CG; ++k) t += part[k][pl];
    cam[b * P + p] = (relu && !(t > 0.f)) ? 0.f : t;
  }
}

// F.interpolate(mode="trilinear", align_corners=False): the source coordinate of output index d is scale (d + 0.5) - 0.5 with scale =
// in / out in fp32, clamped at 0; i0 its floor, i1 = i0 + 1 clamped to in - 1, l1 = the fraction, l0 = 1 - l1
__device__ __forceinline__ void cam_source(int d, float scale, int in, int* i0, int* i1, float* l0, float* l1) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  int k = (int)s;
  k = k < in - 1 ? k : in - 1;
  *i0 = k;
  *i1 = k + (k < in - 1 ? 1 : 0);
  *l1 = s - (float)k;
  *l0 = 1.f - *l1;
}

__global__ __launch_bounds__(CAM_THREADS) void cam_upsample_kernel(const float* __restrict__ cam, int64_t total, int gt, int gh, int gw, int T, int H, int W,
                                                                   float st, float sh, float sw, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * CAM_THREADS + threadIdx.x;
  if (idx >= total) return;
  int64_t q = idx;
  const int x = (int)(q % W); q /= W;
  const int y = (int)(q % H); q /= H;
  const int t = (int)(q % T);
  const int64_t b = q / T;
  int t0, t1, h0, h1, w0, w1;
  float lt0, lt1, lh0, lh1, lw0, lw1;
  cam_source(t, st, gt, &t0, &t1, &lt0, &lt1);
  cam_source(y, sh, gh, &h0, &h1, &lh0, &lh1);
  cam_source(x, sw, gw, &w0, &w1, &lw0, &lw1);
  const float* c = cam + b * gt * gh * gw;
  auto at = [&](int i, int j, int k) { return c[((int64_t)i * gh + j) * gw + k]; };
  const float lo = lh0 * (lw0 * at(t0, h0, w0) + lw1 * at(t0, h0, w1)) + lh1 * (lw0 * at(t0, h1, w0) + lw1 * at(t0, h1, w1));
  const float hi = lh0 * (lw0 * at(t1, h0, w0) + lw1 * at(t1, h0, w1)) + lh1 * (lw0 * at(t1, h1, w0) + lw1 * at(t1, h1, w1));
  out[idx] = lt0 * lo + lt1 * hi;
}

// the shape of a weights / map call: B >= 0, P and C >= 1, every tensor below 2^31 elements
const char* cam_shape(int64_t B, int64_t P, int64_t C) {
  if (B < 0 || P < 1 || C < 1 || B > CAM_MAX || P > CAM_MAX || C > CAM_MAX) return "B >= 0, P >= 1 and C >= 1";
  if (P > CAM_MAX / C || (B > 0 && P * C > CAM_MAX / B)) return "a tensor of 2^31 elements or more";
  return nullptr;
}

int64_t cam_chunks(int64_t P) { return (P + CAM_CHUNK - 1) / CAM_CHUNK; }

bool cam_layout_ok(int layout) { return layout == STLT_CAM_NDHWC || layout == STLT_CAM_NCDHW; }

}  // namespace

extern "C" {

size_t stlt_cam_scratch_bytes(int64_t B, int64_t P, int64_t C) {
  if (cam_shape(B, P, C)) return 0;
  const int64_t chunks = cam_chunks(P);
  return chunks > 1 ? (size_t)B * (size_t)chunks * (size_t)C * sizeof(float) : 0;
}

int stlt_cam_weights(const float* g, int64_t B, int64_t P, int64_t C, int layout, float* alpha, void* scratch, size_t scratch_bytes, stlt_stream_t stream) {
  if (const char* why = cam_shape(B, P, C)) return stlt_set_error(STLT_EINVAL, "stlt_cam_weights: %s (B=%lld, P=%lld, C=%lld)", why, (long long)B, (long long)P, (long long)C);
  if (!cam_layout_ok(layout)) return stlt_set_error(STLT_EINVAL, "stlt_cam_weights: layout is STLT_CAM_NDHWC or STLT_CAM_NCDHW, got %d", layout);
  if (B == 0) return 0;
  if (!g || !alpha) return stlt_set_error(STLT_EINVAL, "stlt_cam_weights: null pointer");
  if ((reinterpret_cast<uintptr_t>(g) & 3) || (reinterpret_cast<uintptr_t>(alpha) & 3)) return stlt_set_error(STLT_EINVAL, "stlt_cam_weights: g and alpha must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("cam_weights B=%lld P=%lld C=%lld layout=%d", (long long)B, (long long)P, (long long)C, layout);
  if (layout == STLT_CAM_NCDHW) {
    const int64_t rows = B * C;
    hipLaunchKernelGGL(cam_weights_ncdhw_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(CAM_THREADS), 0, s, g, rows, (int)P, alpha);
    return stlt_check_launch("cam_weights_ncdhw_kernel");
  }
  const int64_t chunks = cam_chunks(P);
  const size_t need = chunks > 1 ? (size_t)B * (size_t)chunks * (size_t)C * sizeof(float) : 0;
  if (need && (!scratch || scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 15)))
    return stlt_set_error(STLT_EWORKSPACE, "stlt_cam_weights: scratch of %zu bytes, %zu needed (stlt_cam_scratch_bytes), 16-byte aligned", scratch_bytes, need);
  if (B > 65535 || (chunks + 3) / 4 > 65535) return stlt_set_error(STLT_EINVAL, "stlt_cam_weights: more than 65535 clips or 2^23 positions in NDHWC");
  float* out = chunks > 1 ? static_cast<float*>(scratch) : alpha;
  // 16-byte loads and stores: channel quads, with every row of g and of the destination on 16 bytes
  const bool vec = C % 4 == 0 && !(reinterpret_cast<uintptr_t>(g) & 15) && !(reinterpret_cast<uintptr_t>(out) & 15);
  const int64_t cols = vec ? C / 4 : C;
  const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((chunks + 3) / 4), (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(cam_weights_ndhwc_kernel<true>, grid, dim3(CAM_THREADS), 0, s, g, (int)P, (int)C, (int)cols, (int)chunks, out);
  else
    hipLaunchKernelGGL(cam_weights_ndhwc_kernel<false>, grid, dim3(CAM_THREADS), 0, s, g, (int)P, (int)C, (int)cols, (int)chunks, out);
  if (int rc = stlt_check_launch("cam_weights_ndhwc_kernel")) return rc;
  if (chunks == 1) return 0;
  hipLaunchKernelGGL(cam_weights_finish_kernel, dim3((unsigned)((B * C + CAM_THREADS - 1) / CAM_THREADS)), dim3(CAM_THREADS), 0, s, out, B, (int)P, (int)C, (int)chunks, alpha);
  return stlt_check_launch("cam_weights_finish_kernel");
}

int stlt_cam_map(const float* a, const float* w, int per_element, int64_t B, int64_t P, int64_t C, int layout, int relu, float* cam, stlt_stream_t stream) {
  if (const char* why = cam_shape(B, P, C)) return stlt_set_error(STLT_EINVAL, "stlt_cam_map: %s (B=%lld, P=%lld, C=%lld)", why, (long long)B, (long long)P, (long long)C);
  if (!cam_layout_ok(layout)) return stlt_set_error(STLT_EINVAL, "stlt_cam_map: layout is STLT_CAM_NDHWC or STLT_CAM_NCDHW, got %d", layout);
  if (B == 0) return 0;
  if (!a || !w || !cam) return stlt_set_error(STLT_EINVAL, "stlt_cam_map: null pointer");
  if ((reinterpret_cast<uintptr_t>(a) & 3) || (reinterpret_cast<uintptr_t>(w) & 3) || (reinterpret_cast<uintptr_t>(cam) & 3))
    return stlt_set_error(STLT_EINVAL, "stlt_cam_map: a, w and cam must be 4-byte aligned");
  const bool per = per_element != 0;
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("cam_map B=%lld P=%lld C=%lld layout=%d per_element=%d relu=%d", (long long)B, (long long)P, (long long)C, layout, (int)per, relu);
  if (layout == STLT_CAM_NCDHW) {
    if (B > 65535) return stlt_set_error(STLT_EINVAL, "stlt_cam_map: more than 65535 clips in NCDHW");
    const dim3 grid((unsigned)((P + CAM_PT - 1) / CAM_PT), (unsigned)B);
    if (per)
      hipLaunchKernelGGL(cam_map_ncdhw_kernel<true>, grid, dim3(CAM_PT * CAM_CG), 0, s, a, w, (int)P, (int)C, relu, cam);
    else
      hipLaunchKernelGGL(cam_map_ncdhw_kernel<false>, grid, dim3(CAM_PT * CAM_CG), 0, s, a, w, (int)P, (int)C, relu, cam);
    return stlt_check_launch("cam_map_ncdhw_kernel");
  }
  const int64_t positions = B * P;
  const bool vec = C % 4 == 0 && !(reinterpret_cast<uintptr_t>(a) & 15) && !(reinterpret_cast<uintptr_t>(w) & 15);
  const dim3 grid((unsigned)((positions + 3) / 4));
  if (vec && per)
    hipLaunchKernelGGL((cam_map_ndhwc_kernel<true, true>), grid, dim3(CAM_THREADS), 0, s, a, w, positions, (int)P, (int)C, relu, cam);
  else if (vec)
    hipLaunchKernelGGL((cam_map_ndhwc_kernel<true, false>), grid, dim3(CAM_THREADS), 0, s, a, w, positions, (int)P, (int)C, relu, cam);
  else if (per)
    hipLaunchKernelGGL((cam_map_ndhwc_kernel<false, true>), grid, dim3(CAM_THREADS), 0, s, a, w, positions, (int)P, (int)C, relu, cam);
  else
    hipLaunchKernelGGL((cam_map_ndhwc_kernel<false, false>), grid, dim3(CAM_THREADS), 0, s, a, w, positions, (int)P, (int)C, relu, cam);
  return stlt_check_launch("cam_map_ndhwc_kernel");
}

int stlt_cam_upsample(const float* cam, int64_t B, int64_t gt, int64_t gh, int64_t gw, int64_t T, int64_t H, int64_t W, float* out, stlt_stream_t stream) {
  if (B < 0 || B > CAM_MAX || gt < 1 || gh < 1 || gw < 1 || T < 1 || H < 1 || W < 1 || gt > 65536 || gh > 65536 || gw > 65536 || T > 65536 || H > 65536 || W > 65536 ||
      gt * gh * gw > CAM_MAX || (B > 0 && (gt * gh * gw > CAM_MAX / B || T * H > CAM_MAX / W || T * H * W > CAM_MAX / B)))
    return stlt_set_error(STLT_EINVAL, "stlt_cam_upsample: bad shape (B=%lld, grid (%lld,%lld,%lld), output (%lld,%lld,%lld)): extents from 1 to 65536, tensors below 2^31 elements",
                          (long long)B, (long long)gt, (long long)gh, (long long)gw, (long long)T, (long long)H, (long long)W);
  if (B == 0) return 0;
  if (!cam || !out) return stlt_set_error(STLT_EINVAL, "stlt_cam_upsample: null pointer");
  if ((reinterpret_cast<uintptr_t>(cam) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return stlt_set_error(STLT_EINVAL, "stlt_cam_upsample: cam and out must be 4-byte aligned");
  const int64_t total = B * T * H * W;
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("cam_upsample B=%lld grid=(%lld,%lld,%lld) out=(%lld,%lld,%lld)", (long long)B, (long long)gt, (long long)gh, (long long)gw, (long long)T, (long long)H, (long long)W);
  hipLaunchKernelGGL(cam_upsample_kernel, dim3((unsigned)((total + CAM_THREADS - 1) / CAM_THREADS)), dim3(CAM_THREADS), 0, s, cam, total, (int)gt, (int)gh, (int)gw, (int)T,
                     (int)H, (int)W, (float)gt / (float)T, (float)gh / (float)H, (float)gw / (float)W, out);
  return stlt_check_launch("cam_upsample_kernel");
}

}  // extern "C"
