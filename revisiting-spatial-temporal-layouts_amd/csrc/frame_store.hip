// Device frame store: the reference's appearance pipeline (AppearanceDataset.__getitem__, src/modelling/datasets.py:163-208) split at
// the one step that does not depend on the batch.  The reference resizes every frame on its own before any random transform
// (datasets.py:172-177), and Pillow's result is an 8-bit image: the resized frame is a constant of the dataset.
//
// stlt_frames_resize_fwd (ingest, once per frame): Resize(floor(1.15 S)) alone — Pillow's antialiased bilinear filter as two 8-bit
// passes, horizontal then vertical, each only on an axis whose size changes, from the coefficient tables video.resample_table builds.
// The result is written as uint8 into the packed store.
// stlt_frames_batch_fwd (every batch): per clip T byte offsets into the store (or the spill area behind it) and one descriptor.
// Evaluation stages the rows of the S x S crop in LDS with aligned dword loads (a crop row is 3 S contiguous bytes at any byte
// alignment), then every thread turns 12 bytes (4 pixels) into three float4 stores through the 256-entry normalisation table.
// Training first sums the luma of the whole resized frame after the ops that precede contrast (integer sums: any order gives the
// same), again from dword-staged LDS, then the crop kernel runs VideoColorJitter's four ops in the clip's order before the table.
// The per-pixel arithmetic is video_px.h's, shared with video.hip, so both paths give the same bits.
#pragma clang fp contract(off)
#include "common.h"
#include "video_px.h"

namespace {

constexpr int FS_THREADS = 256;
constexpr int64_t FS_MAX_DIM = 1 << 15;   // frame sides (source and resized)
constexpr int64_t FS_MAX_TAPS = 1 << 12;
constexpr int64_t FS_MAX_S = 1024;        // crop side: a row of the crop is staged in LDS
constexpr int64_t FS_MAX_BYTES = (int64_t)1 << 40;
constexpr int FS_CHUNK_PX = 4 * FS_THREADS;  // pixels per block of the luma pass: 4 per thread
constexpr int FS_CHUNK_DW = FS_CHUNK_PX * 3 / 4;

// ---------------------------------------------------------------------------------------------------------------------- ingest
// One 8-bit resample pass along the middle axis of (outer, in_len, inner) bytes -> (outer, out_len, inner): the horizontal pass sees
// the frames as (n * h, w, 3), the vertical pass as (n, h, rw * 3).  Each thread makes 4 consecutive output bytes.
__global__ __launch_bounds__(FS_THREADS) void fs_pass_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t total,
                                                             int in_len, int out_len, int64_t inner, const int32_t* __restrict__ tab,
                                                             int ksize) {
  const int64_t i0 = ((int64_t)blockIdx.x * FS_THREADS + threadIdx.x) * 4;
  if (i0 >= total) return;
  int64_t k = i0 % inner, r = i0 / inner;
  int64_t o = r % out_len, outer = r / out_len;
  uint32_t packed = 0;
  const int cnt = (int)(total - i0 < 4 ? total - i0 : 4);
  for (int j = 0; j < cnt; ++j) {
    const int first = tab[2 * o], n = tab[2 * o + 1];
    const int32_t* w = tab + 2 * (int64_t)out_len + o * ksize;
    const uint8_t* s = src + (outer * in_len + first) * inner + k;
    int acc = 1 << (VP_PREC - 1);
    for (int t = 0; t < n; ++t) acc += (int)s[t * inner] * w[t];
    packed |= (uint32_t)vp_clip8(acc) << (8 * j);
    if (++k == inner) {
      k = 0;
      if (++o == out_len) {
        o = 0;
        ++outer;
      }
    }
  }
  uint8_t* p = dst + i0;
  if (cnt == 4 && ((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = packed;
  } else {
    for (int j = 0; j < cnt; ++j) p[j] = (uint8_t)(packed >> (8 * j));
  }
}

struct FsResizeLayout {
  size_t tab_x, tab_y, mid, total;
};

FsResizeLayout fs_resize_layout(int64_t n, int64_t h, int64_t w, int64_t rh, int64_t rw, int64_t ksize_x, int64_t ksize_y) {
  FsResizeLayout l;
  l.tab_x = 0;
  l.tab_y = l.tab_x + stlt_align256(w != rw ? (size_t)(rw * (2 + ksize_x)) * sizeof(int32_t) : 0);
  l.mid = l.tab_y + stlt_align256(h != rh ? (size_t)(rh * (2 + ksize_y)) * sizeof(int32_t) : 0);
  l.total = l.mid + stlt_align256(w != rw && h != rh ? (size_t)(n * h * rw * 3) : 0);
  return l;
}

bool fs_resize_shape_ok(int64_t n, int64_t h, int64_t w, int64_t rh, int64_t rw, int64_t ksize_x, int64_t ksize_y) {
  if (n <= 0 || h <= 0 || w <= 0 || rh <= 0 || rw <= 0 || h > FS_MAX_DIM || w > FS_MAX_DIM || rh > FS_MAX_DIM || rw > FS_MAX_DIM) return false;
  if (n > FS_MAX_BYTES / (3 * h * w) || n > FS_MAX_BYTES / (3 * rh * rw) || n > FS_MAX_BYTES / (3 * h * rw)) return false;
  if (w != rw && (ksize_x < 1 || ksize_x > FS_MAX_TAPS)) return false;
  if (h != rh && (ksize_y < 1 || ksize_y > FS_MAX_TAPS)) return false;
  return true;
}

// a resample table: every (first, count) pair stays inside the source axis and the row of taps
int fs_check_table(const char* axis, const int32_t* tab, int64_t ksize, int64_t in, int64_t out) {
  if (!tab) return stlt_set_error(STLT_EINVAL, "stlt_frames_resize_fwd: the %s axis changes its size but has no table", axis);
  for (int64_t i = 0; i < out; ++i) {
    const int64_t first = tab[2 * i], count = tab[2 * i + 1];
    if (first < 0 || count < 0 || count > ksize || first + count > in)
      return stlt_set_error(STLT_EINVAL, "stlt_frames_resize_fwd: %s table entry %lld out of range", axis, (long long)i);
  }
  return 0;
}

int fs_launch_pass(const uint8_t* src, uint8_t* dst, int64_t outer, int64_t in_len, int64_t out_len, int64_t inner, const int32_t* tab,
                   int64_t ksize, hipStream_t s) {
  const int64_t total = outer * out_len * inner;
  const int64_t per_block = (int64_t)FS_THREADS * 4;
  hipLaunchKernelGGL(fs_pass_kernel, dim3((unsigned)((total + per_block - 1) / per_block)), dim3(FS_THREADS), 0, s, src, dst, total, (int)in_len,
                     (int)out_len, inner, tab, (int)ksize);
  return stlt_check_launch("fs_pass_kernel");
}

// ----------------------------------------------------------------------------------------------------------------------- batch
__device__ inline const uint8_t* fs_frame(const uint8_t* __restrict__ store, int64_t store_bytes, const uint8_t* __restrict__ spill, int64_t off) {
  return off < store_bytes ? store + off : spill + (off - store_bytes);
}

// 4 bytes starting `sh` bytes into the dword pair (lo, hi)
__device__ inline uint32_t fs_align_bytes(uint32_t hi, uint32_t lo, int sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)); }

// pixels 4 q .. 4 q + 3 of a staged row (the row's first byte lies `sh` bytes into dword 0)
__device__ inline void fs_quad(const uint32_t* __restrict__ row, int q, int sh, Px (&px)[4]) {
  const uint32_t d0 = row[3 * q], d1 = row[3 * q + 1], d2 = row[3 * q + 2], d3 = row[3 * q + 3];
  const uint32_t w[3] = {fs_align_bytes(d1, d0, sh), fs_align_bytes(d2, d1, sh), fs_align_bytes(d3, d2, sh)};
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int byte = 3 * j + c;
      px[j].c[c] = (int)((w[byte >> 2] >> (8 * (byte & 3))) & 255u);
    }
}

// training: per frame, the sum of L over the whole resized frame after the ops that precede contrast
__global__ __launch_bounds__(FS_THREADS) void fs_lsum_kernel(const uint8_t* __restrict__ store, int64_t store_bytes, const uint8_t* __restrict__ spill,
                                                             const int64_t* __restrict__ offs, const stlt_frames_clip* __restrict__ clips, int T,
                                                             unsigned long long* __restrict__ sums) {
  __shared__ uint32_t buf[FS_CHUNK_DW + 2];
  __shared__ unsigned int part;
  const int t = blockIdx.y, b = blockIdx.z;
  const stlt_frames_clip& d = clips[b];  // read in place: order[] is indexed at run time
  const int64_t nbytes = (int64_t)d.rh * d.rw * 3;
  const int64_t c0 = (int64_t)blockIdx.x * FS_CHUNK_PX * 3;
  if (!d.jitter || c0 >= nbytes) return;  // whole block leaves together
  const uintptr_t a = (uintptr_t)(fs_frame(store, store_bytes, spill, offs[(int64_t)b * T + t]) + c0);
  const int sh = (int)(a & 3);
  const int cbytes = (int)(nbytes - c0 < FS_CHUNK_PX * 3 ? nbytes - c0 : FS_CHUNK_PX * 3);
  const int ndw = (sh + cbytes + 3) >> 2;  // <= FS_CHUNK_DW + 1; the last dword ends inside the 4-byte padded buffer
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a - sh);
  for (int i = threadIdx.x; i < ndw; i += FS_THREADS) buf[i] = q[i];
  if (threadIdx.x == 0) part = 0;
  __syncthreads();
  const int npx = cbytes / 3, cpos = vp_contrast_pos(d);
  Px px[4];
  fs_quad(buf, threadIdx.x, sh, px);  // dwords past ndw hold anything: their pixels are not counted
  unsigned int s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (4 * (int)threadIdx.x + j < npx) s += (unsigned int)vp_luma(vp_jitter(px[j], d, 0, cpos, 0));
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(&part, s);
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&sums[(int64_t)b * T + t], (unsigned long long)part);
}

// crop -> (jitter) -> ToTensor + Normalize, stored as (B, 3, T, S, S).  One block: `rows` rows of one frame's crop.
template <bool JITTER>
__global__ __launch_bounds__(FS_THREADS) void fs_out_kernel(const uint8_t* __restrict__ store, int64_t store_bytes, const uint8_t* __restrict__ spill,
                                                            const int64_t* __restrict__ offs, const stlt_frames_clip* __restrict__ clips,
                                                            const float* __restrict__ lut, const unsigned long long* __restrict__ sums, int T, int S,
                                                            int rows, int pitch, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t fs_lds[];  // rows x pitch dwords of crop rows, then the 256-entry table
  float* slut = reinterpret_cast<float*>(fs_lds + rows * pitch);
  const int t = blockIdx.y, b = blockIdx.z, y0 = blockIdx.x * rows;
  const stlt_frames_clip& d = clips[b];  // read in place: order[] is indexed at run time
  const uint8_t* frame = fs_frame(store, store_bytes, spill, offs[(int64_t)b * T + t]);
  const int nrows = min(rows, S - y0);
  const int64_t stride = (int64_t)d.rw * 3;
  const uint8_t* first = frame + ((int64_t)(d.top + y0) * d.rw + d.left) * 3;  // byte (y0, 0, 0) of the crop
  slut[threadIdx.x] = lut[threadIdx.x];
  for (int idx = threadIdx.x; idx < nrows * pitch; idx += FS_THREADS) {
    const int r = idx / pitch, i = idx - r * pitch;
    const uintptr_t a = (uintptr_t)(first + r * stride);
    const int sh = (int)(a & 3);
    if (i < ((sh + 3 * S + 3) >> 2)) fs_lds[idx] = reinterpret_cast<const uint32_t*>(a - sh)[i];  // ends inside the 4-byte padded buffer
  }
  __syncthreads();
  int mean = 0;
  if (JITTER && d.jitter)  // ImageStat: mean = float64 sum / count; Contrast: int(mean + 0.5)
    mean = (int)((double)sums[(int64_t)b * T + t] / (double)((int64_t)d.rh * d.rw) + 0.5);
  const int Q = (S + 3) >> 2;
  const int64_t plane = (int64_t)T * S * S;
  float* o_frame = out + (int64_t)b * 3 * plane + (int64_t)t * S * S;
  for (int idx = threadIdx.x; idx < nrows * Q; idx += FS_THREADS) {
    const int r = idx / Q, q = idx - r * Q;
    const int sh = (int)((uintptr_t)(first + r * stride) & 3);
    Px px[4];
    fs_quad(fs_lds + r * pitch, q, sh, px);  // pixels at x >= S read what the row's tail holds and are not stored
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (JITTER && d.jitter) px[j] = vp_jitter(px[j], d, 0, 4, mean);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][j] = slut[px[j].c[c]];
    }
    float* o = o_frame + (int64_t)(y0 + r) * S + 4 * q;
    if ((S & 3) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * q + j < S) o[c * plane + j] = v[c][j];
    }
  }
}

int fs_check_clip(int64_t b, const stlt_frames_clip& d, int64_t S) {
  if (d.rh <= 0 || d.rw <= 0 || d.rh > FS_MAX_DIM || d.rw > FS_MAX_DIM)
    return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: clip %lld: bad frame size", (long long)b);
  if (d.top < 0 || d.left < 0 || d.top + S > d.rh || d.left + S > d.rw)
    return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: clip %lld: crop outside the resized frame", (long long)b);
  if (d.jitter != 0 && d.jitter != 1) return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: clip %lld: jitter must be 0 or 1", (long long)b);
  if (d.jitter) {
    int seen = 0;
    for (int o = 0; o < 4; ++o) {
      if (d.order[o] < 0 || d.order[o] > 3 || (seen >> d.order[o]) & 1)
        return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: clip %lld: jitter order is not a permutation of 0..3", (long long)b);
      seen |= 1 << d.order[o];
    }
    if (!isfinite(d.brightness) || !isfinite(d.contrast) || !isfinite(d.saturation) || d.hue_shift < 0 || d.hue_shift > 255)
      return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: clip %lld: bad jitter factors", (long long)b);
  }
  return 0;
}

bool fs_batch_shape_ok(int64_t B, int64_t T) { return B > 0 && T > 0 && B <= 65535 && T <= 65535; }

}  // namespace

extern "C" size_t stlt_frames_resize_workspace_bytes(int64_t n, int64_t h, int64_t w, int64_t rh, int64_t rw, int64_t ksize_x, int64_t ksize_y) {
  if (!fs_resize_shape_ok(n, h, w, rh, rw, ksize_x, ksize_y)) return 0;
  const size_t total = fs_resize_layout(n, h, w, rh, rw, ksize_x, ksize_y).total;
  return total ? total : 256;  // never 0 for a good shape
}

extern "C" int stlt_frames_resize_fwd(const uint8_t* src, int64_t n, int64_t h, int64_t w, int64_t rh, int64_t rw, const int32_t* tab_x,
                                      int64_t ksize_x, const int32_t* tab_y, int64_t ksize_y, uint8_t* store, int64_t store_bytes,
                                      int64_t dst_offset, void* workspace, size_t workspace_bytes, stlt_stream_t stream) {
  if (!src || !store || !workspace) return stlt_set_error(STLT_EINVAL, "stlt_frames_resize_fwd: null pointer");
  if (!fs_resize_shape_ok(n, h, w, rh, rw, ksize_x, ksize_y)) return stlt_set_error(STLT_EINVAL, "stlt_frames_resize_fwd: bad shape");
  const int64_t out_bytes = n * rh * rw * 3;
  if (store_bytes <= 0 || dst_offset < 0 || dst_offset > store_bytes || out_bytes > store_bytes - dst_offset)
    return stlt_set_error(STLT_EINVAL, "stlt_frames_resize_fwd: %lld resized bytes at offset %lld do not fit a store of %lld", (long long)out_bytes,
                          (long long)dst_offset, (long long)store_bytes);
  const FsResizeLayout l = fs_resize_layout(n, h, w, rh, rw, ksize_x, ksize_y);
  if (workspace_bytes < l.total) return stlt_set_error(STLT_EINVAL, "stlt_frames_resize_fwd: workspace too small (%zu < %zu)", workspace_bytes, l.total);
  const bool px = w != rw, py = h != rh;  // Pillow runs a pass only on an axis whose size changes
  if (px)
    if (int e = fs_check_table("horizontal", tab_x, ksize_x, w, rw)) return e;
  if (py)
    if (int e = fs_check_table("vertical", tab_y, ksize_y, h, rh)) return e;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* d_tab_x = (int32_t*)(ws + l.tab_x);
  int32_t* d_tab_y = (int32_t*)(ws + l.tab_y);
  uint8_t* mid = (uint8_t*)(ws + l.mid);
  uint8_t* dst = store + dst_offset;
  if (px)
    if (hipError_t e = hipMemcpyAsync(d_tab_x, tab_x, (size_t)(rw * (2 + ksize_x)) * sizeof(int32_t), hipMemcpyHostToDevice, s); e != hipSuccess)
      return stlt_set_error((int)e, "stlt_frames_resize_fwd: table copy: %s", hipGetErrorString(e));
  if (py)
    if (hipError_t e = hipMemcpyAsync(d_tab_y, tab_y, (size_t)(rh * (2 + ksize_y)) * sizeof(int32_t), hipMemcpyHostToDevice, s); e != hipSuccess)
      return stlt_set_error((int)e, "stlt_frames_resize_fwd: table copy: %s", hipGetErrorString(e));
  if (!px && !py) {  // the short side already equals the target: the frames are stored as they are
    if (hipError_t e = hipMemcpyAsync(dst, src, (size_t)out_bytes, hipMemcpyDeviceToDevice, s); e != hipSuccess)
      return stlt_set_error((int)e, "stlt_frames_resize_fwd: frame copy: %s", hipGetErrorString(e));
    return 0;
  }
  if (px)
    if (int e = fs_launch_pass(src, py ? mid : dst, n * h, w, rw, 3, d_tab_x, ksize_x, s)) return e;
  if (py)
    if (int e = fs_launch_pass(px ? mid : src, dst, n, h, rh, rw * 3, d_tab_y, ksize_y, s)) return e;
  return 0;
}

extern "C" size_t stlt_frames_batch_block_bytes(int64_t B, int64_t T) {
  if (!fs_batch_shape_ok(B, T)) return 0;
  return (size_t)(B * T) * sizeof(int64_t) + (size_t)B * sizeof(stlt_frames_clip);
}

extern "C" int stlt_frames_batch_fwd(const uint8_t* store, int64_t store_bytes, const uint8_t* spill, int64_t spill_bytes, const void* batch_host,
                                     void* batch_dev, const float* lut, int64_t B, int64_t T, int64_t S, uint64_t* sums, float* out,
                                     stlt_stream_t stream) {
  if (!batch_host || !batch_dev || !lut || !out) return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: null pointer");
  if (!fs_batch_shape_ok(B, T) || S <= 0 || S > FS_MAX_S) return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: bad shape");
  if (store_bytes < 0 || spill_bytes < 0 || store_bytes > FS_MAX_BYTES || spill_bytes > FS_MAX_BYTES || (store_bytes && !store) ||
      (spill_bytes && !spill))
    return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: bad store / spill size");
  // rows are read as whole aligned dwords: both buffers start on a dword and their sizes are padded to one
  if (((uintptr_t)store & 3) || ((uintptr_t)spill & 3) || (store_bytes & 3) || (spill_bytes & 3) || ((uintptr_t)out & 15) || ((uintptr_t)batch_host & 7) ||
      ((uintptr_t)batch_dev & 7))
    return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: store / spill need 4-byte alignment and padding, out 16-byte, the batch block 8-byte");
  const int64_t* offs = (const int64_t*)batch_host;
  const stlt_frames_clip* clips = (const stlt_frames_clip*)(offs + B * T);
  bool jitter = false;
  int64_t max_bytes = 0;
  for (int64_t b = 0; b < B; ++b) {  // every descriptor and offset is checked before anything is copied or launched
    const stlt_frames_clip& d = clips[b];
    if (int e = fs_check_clip(b, d, S)) return e;
    const int64_t fb = (int64_t)d.rh * d.rw * 3;
    for (int64_t t = 0; t < T; ++t) {
      const int64_t o = offs[b * T + t];
      const bool in_store = o >= 0 && o < store_bytes && fb <= store_bytes - o;
      const bool in_spill = o >= store_bytes && o - store_bytes < spill_bytes && fb <= spill_bytes - (o - store_bytes);
      if (!in_store && !in_spill)
        return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: clip %lld frame %lld: offset %lld outside the store and the spill area", (long long)b,
                              (long long)t, (long long)o);
    }
    jitter |= d.jitter != 0;
    if (fb > max_bytes) max_bytes = fb;
  }
  if (jitter && !sums) return stlt_set_error(STLT_EINVAL, "stlt_frames_batch_fwd: a jittered batch needs the sums buffer");
  hipStream_t s = (hipStream_t)stream;
  if (hipError_t e = hipMemcpyAsync(batch_dev, batch_host, stlt_frames_batch_block_bytes(B, T), hipMemcpyHostToDevice, s); e != hipSuccess)
    return stlt_set_error((int)e, "stlt_frames_batch_fwd: descriptor copy: %s", hipGetErrorString(e));
  const int64_t* d_offs = (const int64_t*)batch_dev;
  const stlt_frames_clip* d_clips = (const stlt_frames_clip*)(d_offs + B * T);
  const unsigned long long* d_sums = (const unsigned long long*)sums;
  if (jitter) {
    if (hipError_t e = hipMemsetAsync(sums, 0, (size_t)(B * T) * sizeof(uint64_t), s); e != hipSuccess)
      return stlt_set_error((int)e, "stlt_frames_batch_fwd: memset: %s", hipGetErrorString(e));
    const int64_t chunk = (int64_t)FS_CHUNK_PX * 3;
    hipLaunchKernelGGL(fs_lsum_kernel, dim3((unsigned)((max_bytes + chunk - 1) / chunk), (unsigned)T, (unsigned)B), dim3(FS_THREADS), 0, s, store,
                       store_bytes, spill, d_offs, d_clips, (int)T, (unsigned long long*)sums);
    if (int e = stlt_check_launch("fs_lsum_kernel")) return e;
  }
  const int Q = (int)((S + 3) >> 2);
  const int pitch = 3 * Q + 1;                                 // dwords per staged row: 3 S bytes at any alignment, plus the quad reader's look-ahead
  const int rows = (int)(S < 16 ? S : (pitch > 512 ? 8192 / pitch : 16));  // <= 32 KiB of rows
  const size_t lds = (size_t)rows * pitch * sizeof(uint32_t) + 256 * sizeof(float);
  const dim3 grid((unsigned)((S + rows - 1) / rows), (unsigned)T, (unsigned)B);
  if (jitter)
    hipLaunchKernelGGL(fs_out_kernel<true>, grid, dim3(FS_THREADS), lds, s, store, store_bytes, spill, d_offs, d_clips, lut, d_sums, (int)T, (int)S, rows,
                       pitch, out);
  else
    hipLaunchKernelGGL(fs_out_kernel<false>, grid, dim3(FS_THREADS), lds, s, store, store_bytes, spill, d_offs, d_clips, lut, d_sums, (int)T, (int)S, rows,
                       pitch, out);
  return stlt_check_launch("fs_out_kernel");
}
