// Device video collater: the reference's per-frame clip transforms (AppearanceDataset.__getitem__, src/modelling/datasets.py:163-208:
// Resize(floor(1.15 S)) -> VideoColorJitter in training (src/utils/data_utils.py:110-137) -> RandomCrop / center_crop -> ToTensor +
// Normalize(0.5, 0.5)) on decoded uint8 frames, restated from Pillow's 8-bit code so that the result is the reference's bit for bit.
//
// Per output pixel the resample is recomputed from the source (no intermediate image): Pillow's horizontal pass (rounded to uint8)
// over the rows in the vertical support, then the vertical pass — each pass only where Pillow runs it, i.e. on an axis whose size
// changes.  The coefficient tables (bounds and 22-fraction-bit weights) come from the host, computed in float64 in Pillow's order.
// Evaluation is one launch over the S x S crops.  Training needs the mean luma of the whole resized frame after the ops that precede
// contrast (ImageEnhance.Contrast), so one launch first sums it per frame (integer sums: any order gives the same), then the crop
// launch runs the four ops in the clip's order and stores.  Blends are Image.blend's float32 arithmetic; HSV follows
// libImaging/Convert.c (float32 variables, float64 literals).  No contraction anywhere below.
#pragma clang fp contract(off)
#include "common.h"
#include "video_px.h"

namespace {

constexpr int VP_THREADS = 256;

// horizontal pass of one source row at resized column x (or the source pixel when the axis keeps its size)
__device__ inline Px vp_hpass(const uint8_t* __restrict__ row, const stlt_video_clip& d, const int32_t* __restrict__ tab, int x) {
  Px p;
  if (d.tab_x < 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p.c[c] = row[(int64_t)x * 3 + c];
    return p;
  }
  const int32_t* b = tab + d.tab_x + 2 * x;
  const int32_t* k = tab + d.tab_x + 2 * d.rw + (int64_t)x * d.ksize_x;
  const int xmin = b[0], n = b[1];
  int acc[3] = {1 << (VP_PREC - 1), 1 << (VP_PREC - 1), 1 << (VP_PREC - 1)};
  const uint8_t* s = row + (int64_t)xmin * 3;
  for (int i = 0; i < n; ++i) {
    const int w = k[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += (int)s[i * 3 + c] * w;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) p.c[c] = vp_clip8(acc[c]);
  return p;
}

// pixel (y, x) of the resized frame
__device__ inline Px vp_resized(const uint8_t* __restrict__ frame, const stlt_video_clip& d, const int32_t* __restrict__ tab, int y,
                                int x) {
  const int64_t stride = (int64_t)d.w * 3;
  if (d.tab_y < 0) return vp_hpass(frame + y * stride, d, tab, x);
  const int32_t* b = tab + d.tab_y + 2 * y;
  const int32_t* k = tab + d.tab_y + 2 * d.rh + (int64_t)y * d.ksize_y;
  const int ymin = b[0], n = b[1];
  int acc[3] = {1 << (VP_PREC - 1), 1 << (VP_PREC - 1), 1 << (VP_PREC - 1)};
  for (int j = 0; j < n; ++j) {
    const Px h = vp_hpass(frame + (ymin + j) * stride, d, tab, x);
    const int w = k[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += h.c[c] * w;
  }
  Px p;
#pragma unroll
  for (int c = 0; c < 3; ++c) p.c[c] = vp_clip8(acc[c]);
  return p;
}

// training: per frame, the sum of L over the whole resized frame after the ops that precede contrast
__global__ __launch_bounds__(VP_THREADS) void video_lsum_kernel(const uint8_t* __restrict__ frames, const stlt_video_clip* __restrict__ clips,
                                                                const int32_t* __restrict__ tab, int T,
                                                                unsigned long long* __restrict__ sums) {
  __shared__ unsigned int part;
  const int t = blockIdx.y, b = blockIdx.z;
  const stlt_video_clip& d = clips[b];  // read in place: order[] is indexed at run time
  const int npix = d.rh * d.rw;
  const int p0 = blockIdx.x * VP_THREADS;
  if (!d.jitter || p0 >= npix) return;  // whole block leaves together
  if (threadIdx.x == 0) part = 0;
  __syncthreads();
  const int pix = p0 + threadIdx.x;
  if (pix < npix) {
    const uint8_t* frame = frames + d.src_offset + (int64_t)t * d.h * d.w * 3;
    const Px p = vp_jitter(vp_resized(frame, d, tab, pix / d.rw, pix % d.rw), d, 0, vp_contrast_pos(d), 0);
    atomicAdd(&part, (unsigned int)vp_luma(p));
  }
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&sums[(int64_t)b * T + t], (unsigned long long)part);
}

// crop -> (jitter) -> ToTensor + Normalize, stored as (B, 3, T, S, S)
__global__ __launch_bounds__(VP_THREADS) void video_out_kernel(const uint8_t* __restrict__ frames, const stlt_video_clip* __restrict__ clips,
                                                               const int32_t* __restrict__ tab, const float* __restrict__ lut,
                                                               const unsigned long long* __restrict__ sums, int T, int S,
                                                               float* __restrict__ out) {
  const int t = blockIdx.y, b = blockIdx.z;
  const int pix = blockIdx.x * VP_THREADS + threadIdx.x;
  if (pix >= S * S) return;
  const stlt_video_clip& d = clips[b];  // read in place: order[] is indexed at run time
  const int y = pix / S, x = pix % S;
  const uint8_t* frame = frames + d.src_offset + (int64_t)t * d.h * d.w * 3;
  Px p = vp_resized(frame, d, tab, d.top + y, d.left + x);
  if (d.jitter) {
    // ImageStat: mean = float64 sum / count; Contrast: int(mean + 0.5)
    const int mean = (int)((double)sums[(int64_t)b * T + t] / (double)((int64_t)d.rh * d.rw) + 0.5);
    p = vp_jitter(p, d, 0, 4, mean);
  }
  const int64_t plane = (int64_t)T * S * S;
  float* o = out + (int64_t)b * 3 * plane + (int64_t)t * S * S + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * plane] = lut[p.c[c]];
}

struct VpLayout {
  size_t clips, tables, lut, sums, total;
};

VpLayout vp_layout(int64_t B, int64_t T, int64_t n_table) {
  VpLayout l;
  l.clips = 0;
  l.tables = l.clips + stlt_align256((size_t)B * sizeof(stlt_video_clip));
  l.lut = l.tables + stlt_align256((size_t)n_table * sizeof(int32_t));
  l.sums = l.lut + stlt_align256(256 * sizeof(float));
  l.total = l.sums + stlt_align256((size_t)B * T * sizeof(unsigned long long));
  return l;
}

constexpr int64_t VP_MAX_DIM = 1 << 15;  // frame sides (source and resized)
constexpr int64_t VP_MAX_TAPS = 1 << 12;

// one axis: no table exactly when the size stays (Pillow runs no pass there); otherwise the table must lie in tables[0, n_table)
// and every (first, count) pair must stay inside the source axis and the row of taps
int vp_check_axis(const char* axis, int64_t b, int32_t off, int32_t ksize, int64_t in, int64_t out, const int32_t* tables,
                  int64_t n_table) {
  if (in == out) {
    if (off != -1) return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: %s axis keeps its size but has a table", (long long)b, axis);
    return 0;
  }
  if (off < 0 || ksize < 1 || ksize > VP_MAX_TAPS || !tables || off + out * (2 + ksize) > n_table)
    return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: %s table outside the table buffer", (long long)b, axis);
  for (int64_t i = 0; i < out; ++i) {
    const int64_t first = tables[off + 2 * i], count = tables[off + 2 * i + 1];
    if (first < 0 || count < 0 || count > ksize || first + count > in)
      return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: %s table entry %lld out of range", (long long)b, axis, (long long)i);
  }
  return 0;
}

int vp_check_clip(int64_t b, const stlt_video_clip& d, int64_t T, int64_t S, int64_t frames_bytes, const int32_t* tables,
                  int64_t n_table) {
  if (d.h <= 0 || d.w <= 0 || d.rh <= 0 || d.rw <= 0 || d.h > VP_MAX_DIM || d.w > VP_MAX_DIM || d.rh > VP_MAX_DIM || d.rw > VP_MAX_DIM)
    return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: bad frame size", (long long)b);
  if (d.top < 0 || d.left < 0 || d.top + S > d.rh || d.left + S > d.rw)
    return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: crop outside the resized frame", (long long)b);
  const int64_t bytes = T * d.h * d.w * 3;
  if (d.src_offset < 0 || d.src_offset > frames_bytes || bytes > frames_bytes - d.src_offset)
    return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: frames outside the packed buffer", (long long)b);
  if (int e = vp_check_axis("horizontal", b, d.tab_x, d.ksize_x, d.w, d.rw, tables, n_table)) return e;
  if (int e = vp_check_axis("vertical", b, d.tab_y, d.ksize_y, d.h, d.rh, tables, n_table)) return e;
  if (d.jitter != 0 && d.jitter != 1) return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: jitter must be 0 or 1", (long long)b);
  if (d.jitter) {
    int seen = 0;
    for (int o = 0; o < 4; ++o) {
      if (d.order[o] < 0 || d.order[o] > 3 || (seen >> d.order[o]) & 1)
        return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: jitter order is not a permutation of 0..3", (long long)b);
      seen |= 1 << d.order[o];
    }
    if (!isfinite(d.brightness) || !isfinite(d.contrast) || !isfinite(d.saturation) || d.hue_shift < 0 || d.hue_shift > 255)
      return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: clip %lld: bad jitter factors", (long long)b);
  }
  return 0;
}

}  // namespace

extern "C" size_t stlt_video_prep_workspace_bytes(int64_t B, int64_t T, int64_t n_table) {
  if (B <= 0 || T <= 0 || n_table < 0 || B > 65535 || T > 65535 || n_table > ((int64_t)1 << 40)) return 0;
  return vp_layout(B, T, n_table).total;
}

extern "C" int stlt_video_prep_fwd(const uint8_t* frames, int64_t frames_bytes, const stlt_video_clip* clips, const int32_t* tables,
                                   int64_t n_table, const float* lut, int64_t B, int64_t T, int64_t S, float* out, void* workspace,
                                   size_t workspace_bytes, stlt_stream_t stream) {
  if (!frames || !clips || !lut || !out || !workspace) return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: null pointer");
  if (B <= 0 || T <= 0 || S <= 0 || B > 65535 || T > 65535 || S > VP_MAX_DIM || frames_bytes <= 0 || n_table < 0 || n_table > ((int64_t)1 << 40))
    return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: bad shape");
  const VpLayout l = vp_layout(B, T, n_table);
  if (workspace_bytes < l.total) return stlt_set_error(STLT_EINVAL, "stlt_video_prep_fwd: workspace too small (%zu < %zu)", workspace_bytes, l.total);
  bool jitter = false;
  int64_t max_pix = 0;
  for (int64_t b = 0; b < B; ++b) {  // every descriptor is checked before anything is launched or copied
    if (int e = vp_check_clip(b, clips[b], T, S, frames_bytes, tables, n_table)) return e;
    jitter |= clips[b].jitter != 0;
    const int64_t np_ = (int64_t)clips[b].rh * clips[b].rw;
    if (np_ > max_pix) max_pix = np_;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  stlt_video_clip* d_clips = (stlt_video_clip*)(ws + l.clips);
  int32_t* d_tab = (int32_t*)(ws + l.tables);
  float* d_lut = (float*)(ws + l.lut);
  unsigned long long* d_sums = (unsigned long long*)(ws + l.sums);
  if (hipError_t e = hipMemcpyAsync(d_clips, clips, (size_t)B * sizeof(stlt_video_clip), hipMemcpyHostToDevice, s); e != hipSuccess)
    return stlt_set_error((int)e, "stlt_video_prep_fwd: descriptor copy: %s", hipGetErrorString(e));
  if (n_table > 0)
    if (hipError_t e = hipMemcpyAsync(d_tab, tables, (size_t)n_table * sizeof(int32_t), hipMemcpyHostToDevice, s); e != hipSuccess)
      return stlt_set_error((int)e, "stlt_video_prep_fwd: table copy: %s", hipGetErrorString(e));
  if (hipError_t e = hipMemcpyAsync(d_lut, lut, 256 * sizeof(float), hipMemcpyHostToDevice, s); e != hipSuccess)
    return stlt_set_error((int)e, "stlt_video_prep_fwd: table copy: %s", hipGetErrorString(e));
  if (jitter) {
    if (hipError_t e = hipMemsetAsync(d_sums, 0, (size_t)B * T * sizeof(unsigned long long), s); e != hipSuccess)
      return stlt_set_error((int)e, "stlt_video_prep_fwd: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(video_lsum_kernel, dim3((unsigned)((max_pix + VP_THREADS - 1) / VP_THREADS), (unsigned)T, (unsigned)B), dim3(VP_THREADS), 0, s,
                       frames, d_clips, d_tab, (int)T, d_sums);
    if (int e = stlt_check_launch("video_lsum_kernel")) return e;
  }
  hipLaunchKernelGGL(video_out_kernel, dim3((unsigned)((S * S + VP_THREADS - 1) / VP_THREADS), (unsigned)T, (unsigned)B), dim3(VP_THREADS), 0, s,
                     frames, d_clips, d_tab, d_lut, d_sums, (int)T, (int)S, out);
  return stlt_check_launch("video_out_kernel");
}
