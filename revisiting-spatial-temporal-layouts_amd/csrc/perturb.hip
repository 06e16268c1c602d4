// The perturbation test of an attribution map on the device (Chefer, Gur, Wolf 2021, "positive" and "negative" perturbation): rank the
// real object tokens of every clip by a map, delete the first k of them for a rising k, score the model's logits on each reduced batch.
// A deleted slot is what the reference's dataset and collater make of a slot without a detection (src/modelling/datasets.py:88-93, 274-278:
// category 0, box (0,0,0,0), score 0, key-padding mask True), a frame left without an object gets the frame type "empty"
// (datasets.py:64-69): a perturbed batch is a batch the reference itself could have been handed.
//
//   perturb_rank_kernel   one workgroup per clip: the candidates' packed 64-bit keys (ordered score bits, then flat index) are sorted in LDS
//                         with the bitonic network of eval_ap_kernel (evalk.hip); the index in the low word makes the order total, so the
//                         sort is stable and ties go to the lower index in both orders.  Non-candidates carry the all-ones key and sort last.
//   perturb_apply_kernel  one workgroup per (step, clip): slots whose rank is below the step's count are blanked, every other value is
//                         moved as the integer it is stored as (bit for bit), frames that lost their last object change type.
//   perturb_curve_kernel  one wave per logits row: the stabilised softmax probability (or the sigmoid) of the clip's target class and
//                         whether any class beats it — eval_topk_kernel's rule (larger logit, or equal logit at a lower index).
//   perturb_apply_cells_kernel / cell_pool_kernel  the appearance side (further down): video cells and feature columns set to a fill
//                         value per step, and |gradient| (or the signed attribution) summed per cell.  Cells are ranked by perturb_rank_kernel<true>: the same sort.
#include <cstring>
#include "common.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_MAX_ITEMS = 16384;  // 8-byte keys in LDS: 128 KB
constexpr unsigned long long PT_NONE = ~0ull;

// monotone map float -> uint32 (larger float = larger key) on the canonical value (-0 -> +0); inverted for the descending order, so that an
// ASCENDING key sort is the removal order.  NaN takes the largest 32-bit key in both orders: no other value maps there (+inf / -inf reach
// 0xff800000 at most), and with a flat index below 2^14 in the low word the packed key stays below PT_NONE.
__device__ __forceinline__ uint32_t removal_key(float v, int descending) {
  if (v != v) return 0xffffffffu;
  if (v == 0.f) v = 0.f;
  uint32_t u = __float_as_uint(v);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return descending ? ~u : u;
}

// CELLS: every item is a candidate (the video cells of stlt_perturb_rank_cells: no mask and no lengths are read); the sort is the same code
template <bool CELLS>
__global__ __launch_bounds__(PT_THREADS) void perturb_rank_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ kpm, const int64_t* __restrict__ lengths,
                                                                  int T, int N, int unit_frame, int descending, int n_items, int n_pow2,
                                                                  int* __restrict__ rank, int* __restrict__ n_candidates) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];  // n_pow2 keys
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  int64_t t_end = 0;
  const uint8_t* m = nullptr;
  if constexpr (!CELLS) {
    const int64_t len = lengths[b];
    t_end = len - 1 < (int64_t)T ? len - 1 : (int64_t)T;  // frames [0, t_end) may hold candidates: never the extract frame, never past T
    m = kpm + b * (int64_t)T * N;
  }
  const float* sc = scores + b * (int64_t)n_items;
  int* rk = rank + b * (int64_t)n_items;
  for (int i = tid; i < n_pow2; i += PT_THREADS) {
    unsigned long long k = PT_NONE;
    if (i < n_items) {
      bool cand;
      if constexpr (CELLS) {
        cand = true;
      } else if (unit_frame) {
        cand = false;
        if (i < t_end)
          for (int n = 1; n < N; ++n) cand |= m[(int64_t)i * N + n] == 0;
      } else {
        const int t = i / N, n = i - t * N;
        cand = t < t_end && n >= 1 && m[i] == 0;
      }
      if (cand) k = ((unsigned long long)removal_key(sc[i], descending) << 32) | (unsigned long long)(unsigned)i;
      else rk[i] = -1;  // every entry of rank is written exactly once: here, or below from the sorted keys
    }
    keys[i] = k;
  }
  __syncthreads();
  for (int size = 2; size <= n_pow2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (n_pow2 >> 1); i += PT_THREADS) {
        const int lo = 2 * i - (i & (stride - 1));  // index of the lower element of the i-th pair at this stride
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = keys[lo], c = keys[hi];
        if ((a > c) == up) { keys[lo] = c; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
  // the candidates are the first keys; the one position whose successor is no candidate names their count
  for (int p = tid; p < n_pow2; p += PT_THREADS) {
    const unsigned long long k = keys[p];
    if (k != PT_NONE) {
      rk[(unsigned)(k & 0xffffffffull)] = p;
      if (p + 1 == n_pow2 || keys[p + 1] == PT_NONE) n_candidates[b] = p + 1;
    } else if (p == 0) {
      n_candidates[b] = 0;
    }
  }
}

struct PerturbBatch {  // the tensors of a collated batch (scores may be null), in or out
  int64_t* categories; uint32_t* boxes; uint32_t* scores; uint8_t* kpm_boxes; int64_t* frame_types; uint8_t* kpm_frames; int64_t* lengths;
};

__global__ __launch_bounds__(PT_THREADS) void perturb_apply_kernel(PerturbBatch in, const int* __restrict__ rank, const int* __restrict__ n_candidates,
                                                                   int64_t B, int T, int N, int unit_frame, int64_t steps, int64_t s0,
                                                                   int64_t empty_frame_type, PerturbBatch out, int* __restrict__ removed) {
  const int64_t clip = blockIdx.x;  // (s - s0) * B + b
  const int64_t ds = clip / B, b = clip - ds * B, s = s0 + ds;
  const int tid = threadIdx.x;
  const int64_t k = s * (int64_t)n_candidates[b] / steps;  // floor: step s removes the first k of the removal order
  const int64_t slots = (int64_t)T * N;
  const int* rk = rank + b * (unit_frame ? (int64_t)T : slots);
  const uint8_t* m_in = in.kpm_boxes + b * slots;
  for (int64_t i = tid; i < slots; i += PT_THREADS) {
    const int t = (int)(i / N), n = (int)(i - (int64_t)t * N);
    const uint8_t masked = m_in[i];
    const int r = unit_frame ? ((n >= 1 && masked == 0) ? rk[t] : -1) : rk[i];
    const bool gone = r >= 0 && r < k;
    const int64_t src = b * slots + i, dst = clip * slots + i;
    out.categories[dst] = gone ? 0 : in.categories[src];
#pragma unroll
    for (int c = 0; c < 4; ++c) out.boxes[dst * 4 + c] = gone ? 0u : in.boxes[src * 4 + c];
    if (in.scores) out.scores[dst] = gone ? 0u : in.scores[src];
    out.kpm_boxes[dst] = gone ? (uint8_t)1 : masked;
  }
  for (int t = tid; t < T; t += PT_THREADS) {
    // a frame changes type when it had a candidate and every candidate of it is gone (a frame's real slots n >= 1 are candidates all or none)
    bool had = false, left = false;
    for (int n = 1; n < N; ++n) {
      const int r = unit_frame ? (m_in[(int64_t)t * N + n] == 0 ? rk[t] : -1) : rk[(int64_t)t * N + n];
      had |= r >= 0;
      left |= r >= k;
    }
    const int64_t ft = in.frame_types[b * T + t];
    out.frame_types[clip * T + t] = (had && !left) ? empty_frame_type : ft;
    out.kpm_frames[clip * T + t] = in.kpm_frames[b * T + t];
  }
  if (tid == 0) {
    out.lengths[clip] = in.lengths[b];
    removed[s * B + b] = (int)k;
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// arg-max of a row, first maximum on ties (torch.argmax; eval_topk_kernel's "no class beats it"); a row without any comparable value: 0
__device__ __forceinline__ int wave_argmax(const float* __restrict__ x, int K, int lane) {
  float best = -__builtin_inff();
  int at = 0x7fffffff;
  for (int j = lane; j < K; j += 64) {
    const float v = x[j];
    if (v > best || (v == best && j < at)) { best = v; at = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(at, o, 64);
    if (ov > best || (ov == best && oa < at)) { best = ov; at = oa; }
  }
  return at == 0x7fffffff ? 0 : at;
}

__global__ __launch_bounds__(PT_THREADS) void perturb_curve_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ target, int64_t S,
                                                                   int64_t B, int K, int sigmoid, float* __restrict__ prob, uint8_t* __restrict__ hit,
                                                                   int64_t* __restrict__ target_out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // s * B + b
  if (row >= S * B) return;
  const int64_t b = row % B;
  int64_t y;
  if (target) y = target[b];
  else y = wave_argmax(logits + b * ld, K, lane);  // the clip's step-0 row, found again by every wave that needs it: no launch order between the steps
  if (row < B && target_out && lane == 0) target_out[b] = y;
  if (y < 0 || y >= K) {  // an out-of-range target can never be hit
    if (lane == 0) { prob[row] = 0.f; hit[row] = 0; }
    return;
  }
  const float* x = logits + row * ld;
  const float xy = x[y];
  if (sigmoid) {
    if (lane == 0) { prob[row] = (float)(1.0 / (1.0 + exp(-(double)xy))); hit[row] = xy > 0.f ? 1 : 0; }
    return;
  }
  float mx = -__builtin_inff();
  int beaten_by = 0;
  for (int j0 = 0; j0 < K; j0 += 64) {
    const int j = j0 + lane;
    bool beats = false;
    if (j < K) {
      const float v = x[j];
      mx = fmaxf(mx, v);
      beats = v > xy || (v == xy && j < (int)y);
    }
    beaten_by += __popcll(__ballot(beats));
  }
  mx = wave_max(mx);
  // one probability per row is kept, so the row is summed in float64 (a few hundred exponentials per wave) and rounded once
  double sum = 0.0;
  for (int j = lane; j < K; j += 64) sum += exp((double)x[j] - (double)mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) { prob[row] = (float)(exp((double)xy - (double)mx) / sum); hit[row] = beaten_by == 0 ? 1 : 0; }
}

// ---- the appearance side: video cells (the stride block of one appearance token) and feature columns ----
// The reference's appearance encoder takes no key-padding mask (src/modelling/models.py:269, self.transformer(src=features)), so a token is
// deleted at the input: cell (gt,gh,gw) of video_frames (B,3,T,H,W) — the block the trunk's strides map onto appearance token
// 1 + (gt*Gh + gh)*Gw + gw (features.flatten(2), models.py:260) — is set to `fill`, 0.0 being mid-grey after Normalize(0.5, 0.5)
// (src/modelling/datasets.py:151).  Precomputed appearance_features are the same tensor shape with cells of 1 x 1 x 1.

constexpr int PC_ITEMS = 8;  // lane accesses of one thread of perturb_apply_cells_kernel (a block covers PT_THREADS * PC_ITEMS of them, more when the grid is large)
constexpr int PC_NEVER = 0x7fffffff;

struct CellGeom {  // one clip: (Cch, T, H, W) cut into cells of (ct, ch, cw); the grid is (Gt, Gh, Gw), ragged last cells on every axis
  int Cch, T, H, W, ct, ch, cw, Gh, Gw;
};

// One workgroup per (clip, chunk of the clip's lane accesses).  LDS holds, per cell, the first step at which the cell is deleted,
// ceil((rank+1) * steps / n_candidates) — step s deletes rank < floor(s * n / steps), which is s * n >= (rank+1) * steps — so every source
// element is read once and written s1-s0+1 times, value or fill, on one compare per step.  VEC: 16-byte lane accesses (W % 4 == 0 and
// cw % 4 == 0: the four floats lie in one cell and in one row); otherwise one float per access.
template <bool VEC>
__global__ __launch_bounds__(PT_THREADS) void perturb_apply_cells_kernel(const uint32_t* __restrict__ x, CellGeom g, int C, const int* __restrict__ rank,
                                                                         const int* __restrict__ n_candidates, int64_t B, int64_t steps, int64_t s0, int n_steps,
                                                                         uint32_t fill, uint32_t chunk, uint32_t chunks, uint32_t* __restrict__ out,
                                                                         int* __restrict__ removed) {
  extern __shared__ __attribute__((aligned(16))) int first_step[];  // C entries
  const int64_t b = blockIdx.x / chunks;
  const uint32_t part = blockIdx.x - (uint32_t)b * chunks;
  const int tid = threadIdx.x;
  const int64_t n = n_candidates[b];
  for (int c = tid; c < C; c += PT_THREADS) {
    const int r = rank[b * C + c];
    int f = PC_NEVER;
    if (r >= 0 && n > 0) {
      const int64_t q = ((int64_t)(r + 1) * steps + n - 1) / n;  // (r+1) <= 2^14 and steps < 2^31: the product fits
      f = q < PC_NEVER ? (int)q : PC_NEVER;
    }
    first_step[c] = f;
  }
  if (part == 0 && removed && tid < n_steps) removed[(int64_t)tid * B + b] = (int)((s0 + tid) * n / steps);
  __syncthreads();
  constexpr uint32_t LANE = VEC ? 4 : 1;
  const uint32_t wq = (uint32_t)g.W / LANE;                                         // lane accesses of one row
  const uint32_t items = (uint32_t)g.Cch * (uint32_t)g.T * (uint32_t)g.H * wq;      // ... of one clip (the launcher keeps the element count below 2^31)
  const int64_t clip_elems = (int64_t)items * LANE;
  const uint32_t lo = part * chunk, hi = lo + chunk < items ? lo + chunk : items;   // chunk * chunks < 2^32 (launcher)
  const uint32_t* src = x + b * clip_elems;
  for (uint32_t i = lo + tid; i < hi; i += PT_THREADS) {
    const uint32_t row = i / wq, w = (i - row * wq) * LANE;
    const uint32_t th = row % ((uint32_t)g.T * g.H);  // the channel does not matter: a cell spans them all
    const uint32_t t = th / g.H, h = th - t * g.H;
    const int f = first_step[((t / g.ct) * g.Gh + h / g.ch) * g.Gw + w / g.cw];
    const int64_t off = (int64_t)i * LANE;
    if constexpr (VEC) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + off);
      const uint4 blank = make_uint4(fill, fill, fill, fill);
      for (int ds = 0; ds < n_steps; ++ds)
        *reinterpret_cast<uint4*>(out + ((int64_t)ds * B + b) * clip_elems + off) = (s0 + ds >= f) ? blank : v;
    } else {
      const uint32_t v = src[off];
      for (int ds = 0; ds < n_steps; ++ds) out[((int64_t)ds * B + b) * clip_elems + off] = (s0 + ds >= f) ? fill : v;
    }
  }
}

// One workgroup per (clip, cell): sum of |g| over the cell and all channels in a fixed order — element e of the cell (channel-major, then
// frame, row, column) goes to accumulator (e / PT_THREADS) % 4 of thread e % PT_THREADS; the four are added pairwise, then the wave by
// xor-shuffles, then the four waves in order.  No atomics: the same bits on every launch.  ABS = false is the signed twin (stlt_cell_pool_sum:
// a signed attribution map pooled per cell) — the same order, the value itself in place of its magnitude.
template <bool ABS>
__global__ __launch_bounds__(PT_THREADS) void cell_pool_kernel(const float* __restrict__ gr, CellGeom g, int Gt, float* __restrict__ out) {
  __shared__ float wave_sum[PT_THREADS / 64];
  const int C = Gt * g.Gh * g.Gw;
  const int64_t b = blockIdx.x / C;
  const int c = (int)(blockIdx.x - b * C);
  const int gt = c / (g.Gh * g.Gw), gh = (c / g.Gw) % g.Gh, gw = c % g.Gw;
  const int t0 = gt * g.ct, h0 = gh * g.ch, w0 = gw * g.cw;
  const uint32_t nt = (uint32_t)(g.T - t0 < g.ct ? g.T - t0 : g.ct), nh = (uint32_t)(g.H - h0 < g.ch ? g.H - h0 : g.ch), nw = (uint32_t)(g.W - w0 < g.cw ? g.W - w0 : g.cw);
  const uint32_t per_ch = nt * nh * nw, total = (uint32_t)g.Cch * per_ch;  // <= the clip's element count < 2^31
  const float* base = gr + b * ((int64_t)g.Cch * g.T * g.H * g.W);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t k = 0;
  for (uint32_t e = threadIdx.x; e < total; e += PT_THREADS, k = (k + 1) & 3) {
    const uint32_t ch = e / per_ch, r = e - ch * per_ch;
    const uint32_t dt = r / (nh * nw), r2 = r - dt * (nh * nw);
    const uint32_t dh = r2 / nw, dw = r2 - dh * nw;
    const float raw = base[(((int64_t)ch * g.T + (t0 + dt)) * g.H + (h0 + dh)) * g.W + (w0 + dw)];
    const float v = ABS ? fabsf(raw) : raw;
    acc[0] += k == 0 ? v : 0.f; acc[1] += k == 1 ? v : 0.f; acc[2] += k == 2 ? v : 0.f; acc[3] += k == 3 ? v : 0.f;  // adding +0 changes no bit of a non-negative sum (of a signed one: at most -0 into +0)
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// the shared argument check of the two cell launchers: -> the grid, or an error message
const char* cell_geometry(int64_t B, int64_t Cch, int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, CellGeom* g, int64_t* Gt, int64_t* C) {
  const int64_t lim = 0x7fffffff;
  if (B < 0 || B > lim || Cch <= 0 || T <= 0 || H <= 0 || W <= 0 || Cch > lim || T > lim || H > lim || W > lim) return "bad shape";
  if (ct <= 0 || ch <= 0 || cw <= 0 || ct > lim || ch > lim || cw > lim) return "cell extents must be positive";
  if (Cch > lim / T || Cch * T > lim / H || Cch * T * H > lim / W) return "a clip holds 2^31 elements or more";
  const int64_t gt = (T + ct - 1) / ct, gh = (H + ch - 1) / ch, gw = (W + cw - 1) / cw;
  if (gt > PT_MAX_ITEMS || gh > PT_MAX_ITEMS || gw > PT_MAX_ITEMS || gt * gh > PT_MAX_ITEMS || gt * gh * gw > PT_MAX_ITEMS) return "more cells than a clip is ranked with in LDS";
  *g = CellGeom{(int)Cch, (int)T, (int)H, (int)W, (int)ct, (int)ch, (int)cw, (int)gh, (int)gw};
  *Gt = gt;
  *C = gt * gh * gw;
  return nullptr;
}

// the launcher of stlt_cell_pool_abs and stlt_cell_pool_sum
template <bool ABS>
int cell_pool(const char* who, const float* g, int64_t B, int64_t Cch, int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, float* out, stlt_stream_t stream) {
  CellGeom geom;
  int64_t Gt, C;
  if (const char* why = cell_geometry(B, Cch, T, H, W, ct, ch, cw, &geom, &Gt, &C))
    return stlt_set_error(STLT_EINVAL, "%s: %s (B=%lld, g=(%lld,%lld,%lld,%lld), cells=(%lld,%lld,%lld))", who, why, (long long)B, (long long)Cch, (long long)T,
                          (long long)H, (long long)W, (long long)ct, (long long)ch, (long long)cw);
  if (B == 0) return 0;
  if (B * C > 0x7fffffff) return stlt_set_error(STLT_EINVAL, "%s: %lld workgroups in one call (at most 2^31 - 1)", who, (long long)(B * C));
  if (!g || !out) return stlt_set_error(STLT_EINVAL, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("%s B=%lld g=(%lld,%lld,%lld,%lld) cells=%lld", who + 5, (long long)B, (long long)Cch, (long long)T, (long long)H, (long long)W, (long long)C);
  hipLaunchKernelGGL(cell_pool_kernel<ABS>, dim3((unsigned)(B * C)), dim3(PT_THREADS), 0, s, g, geom, (int)Gt, out);
  return stlt_check_launch(ABS ? "cell_pool_abs_kernel" : "cell_pool_sum_kernel");
}

}  // namespace

extern "C" {

int64_t stlt_perturb_max_items(void) { return PT_MAX_ITEMS; }

int stlt_perturb_rank(const float* scores, const uint8_t* kpm_boxes, const int64_t* lengths, int64_t B, int64_t T, int64_t N, int unit, int descending,
                      int32_t* rank, int32_t* n_candidates, stlt_stream_t stream) {
  if (B < 0 || T <= 0 || N <= 0 || T > PT_MAX_ITEMS || N > PT_MAX_ITEMS || B > 0x7fffffff)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_rank: bad shape (B=%lld, T=%lld, N=%lld)", (long long)B, (long long)T, (long long)N);
  if (T * N > PT_MAX_ITEMS)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_rank: T*N = %lld slots exceed the %d a clip is sorted with in LDS", (long long)(T * N), PT_MAX_ITEMS);
  if ((unit != STLT_PERTURB_OBJECT && unit != STLT_PERTURB_FRAME) || (descending != 0 && descending != 1))
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_rank: unit is 0 (object) or 1 (frame), descending 0 or 1 (got %d, %d)", unit, descending);
  if (B == 0) return 0;  // an empty batch has no storage to point at
  if (!scores || !kpm_boxes || !lengths || !rank || !n_candidates) return stlt_set_error(STLT_EINVAL, "stlt_perturb_rank: null pointer");
  const int n_items = (int)(unit == STLT_PERTURB_FRAME ? T : T * N);
  int n_pow2 = 2;
  while (n_pow2 < n_items) n_pow2 <<= 1;
  const size_t lds = (size_t)n_pow2 * 8;
  static StltPerDeviceOnce once;  // > 64 KB of dynamic LDS needs the attribute, per device
  bool& opted = once.flag();
  if (!opted) {
    if (hipError_t e = hipFuncSetAttribute((const void*)perturb_rank_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, PT_MAX_ITEMS * 8); e != hipSuccess)
      return stlt_set_error((int)e, "stlt_perturb_rank: hipFuncSetAttribute: %s", hipGetErrorString(e));
    opted = true;
  }
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("perturb_rank B=%lld T=%lld N=%lld unit=%d keys=%d", (long long)B, (long long)T, (long long)N, unit, n_pow2);
  hipLaunchKernelGGL(perturb_rank_kernel<false>, dim3((unsigned)B), dim3(PT_THREADS), lds, s, scores, kpm_boxes, lengths, (int)T, (int)N, unit == STLT_PERTURB_FRAME ? 1 : 0,
                     descending, n_items, n_pow2, rank, n_candidates);
  return stlt_check_launch("perturb_rank_kernel");
}

int stlt_perturb_apply(const stlt_inputs* in, const int32_t* rank, const int32_t* n_candidates, int unit, int64_t steps, int64_t s0, int64_t s1,
                       int64_t empty_frame_type, int64_t* categories, float* boxes, float* scores, uint8_t* kpm_boxes, int64_t* frame_types,
                       uint8_t* kpm_frames, int64_t* lengths, int32_t* removed, stlt_stream_t stream) {
  if (!in) return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply: null pointer");
  const int64_t B = in->B, T = in->T, N = in->N;
  if (B < 0 || T <= 0 || N <= 0 || T > 0x7fffffff || N > 0x7fffffff || T > 0x7fffffff / N || B > 0x7fffffff)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply: bad shape (B=%lld, T=%lld, N=%lld)", (long long)B, (long long)T, (long long)N);
  if (unit != STLT_PERTURB_OBJECT && unit != STLT_PERTURB_FRAME) return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply: unit is 0 (object) or 1 (frame), got %d", unit);
  if (steps < 1 || steps > 0x7fffffff || s0 < 0 || s1 < s0 || s1 > steps)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply: steps >= 1 and 0 <= s0 <= s1 <= steps (got steps=%lld, s0=%lld, s1=%lld)", (long long)steps, (long long)s0,
                          (long long)s1);
  if (B == 0) return 0;
  const int64_t clips = (s1 - s0 + 1) * B;
  if (clips > 0x7fffffff) return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply: %lld perturbed clips in one call (at most 2^31 - 1)", (long long)clips);
  if (!in->categories || !in->boxes || !in->kpm_boxes || !in->frame_types || !in->kpm_frames || !in->lengths || !rank || !n_candidates || !categories || !boxes ||
      !kpm_boxes || !frame_types || !kpm_frames || !lengths || !removed || (in->scores && !scores))
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply: null pointer");
  PerturbBatch src{const_cast<int64_t*>(in->categories), reinterpret_cast<uint32_t*>(const_cast<float*>(in->boxes)),
                   reinterpret_cast<uint32_t*>(const_cast<float*>(in->scores)), const_cast<uint8_t*>(in->kpm_boxes), const_cast<int64_t*>(in->frame_types),
                   const_cast<uint8_t*>(in->kpm_frames), const_cast<int64_t*>(in->lengths)};
  PerturbBatch dst{categories, reinterpret_cast<uint32_t*>(boxes), in->scores ? reinterpret_cast<uint32_t*>(scores) : nullptr, kpm_boxes, frame_types, kpm_frames, lengths};
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("perturb_apply B=%lld T=%lld N=%lld unit=%d steps=%lld [%lld,%lld]", (long long)B, (long long)T, (long long)N, unit, (long long)steps, (long long)s0,
                 (long long)s1);
  hipLaunchKernelGGL(perturb_apply_kernel, dim3((unsigned)clips), dim3(PT_THREADS), 0, s, src, rank, n_candidates, B, (int)T, (int)N, unit == STLT_PERTURB_FRAME ? 1 : 0,
                     steps, s0, empty_frame_type, dst, removed);
  return stlt_check_launch("perturb_apply_kernel");
}

int stlt_perturb_curve(const float* logits, int64_t ld, const int64_t* target, int activation, int64_t S, int64_t B, int64_t K, float* prob, uint8_t* hit,
                       int64_t* target_out, stlt_stream_t stream) {
  if (S <= 0 || B < 0 || K <= 0 || K > 0x7fffffff || ld < K || S > 0x7fffffff || B > 0x7fffffff || S * B > (int64_t)0x7fffffff * 4)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_curve: bad shape (S=%lld, B=%lld, K=%lld, ld=%lld)", (long long)S, (long long)B, (long long)K, (long long)ld);
  if (activation != STLT_PERTURB_SOFTMAX && activation != STLT_PERTURB_SIGMOID)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_curve: activation is 0 (softmax) or 1 (sigmoid), got %d", activation);
  if (B == 0) return 0;
  if (!logits || !prob || !hit || (!target && !target_out)) return stlt_set_error(STLT_EINVAL, "stlt_perturb_curve: null pointer (target_out is required when target is NULL)");
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("perturb_curve S=%lld B=%lld K=%lld act=%d", (long long)S, (long long)B, (long long)K, activation);
  hipLaunchKernelGGL(perturb_curve_kernel, dim3((unsigned)((S * B + 3) / 4)), dim3(PT_THREADS), 0, s, logits, ld, target, S, B, (int)K, activation, prob, hit, target_out);
  return stlt_check_launch("perturb_curve_kernel");
}

int stlt_perturb_rank_cells(const float* scores, int64_t B, int64_t C, int descending, int32_t* rank, int32_t* n_candidates, stlt_stream_t stream) {
  if (B < 0 || C <= 0 || B > 0x7fffffff) return stlt_set_error(STLT_EINVAL, "stlt_perturb_rank_cells: bad shape (B=%lld, C=%lld)", (long long)B, (long long)C);
  if (C > PT_MAX_ITEMS)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_rank_cells: C = %lld cells exceed the %d a clip is sorted with in LDS", (long long)C, PT_MAX_ITEMS);
  if (descending != 0 && descending != 1) return stlt_set_error(STLT_EINVAL, "stlt_perturb_rank_cells: descending is 0 or 1, got %d", descending);
  if (B == 0) return 0;
  if (!scores || !rank || !n_candidates) return stlt_set_error(STLT_EINVAL, "stlt_perturb_rank_cells: null pointer");
  int n_pow2 = 2;
  while (n_pow2 < (int)C) n_pow2 <<= 1;
  static StltPerDeviceOnce once;  // > 64 KB of dynamic LDS needs the attribute, per device
  bool& opted = once.flag();
  if (!opted) {
    if (hipError_t e = hipFuncSetAttribute((const void*)perturb_rank_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, PT_MAX_ITEMS * 8); e != hipSuccess)
      return stlt_set_error((int)e, "stlt_perturb_rank_cells: hipFuncSetAttribute: %s", hipGetErrorString(e));
    opted = true;
  }
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("perturb_rank_cells B=%lld C=%lld keys=%d", (long long)B, (long long)C, n_pow2);
  // the cells are one "frame" of C items each: T = 1, N = C, no mask, no lengths
  hipLaunchKernelGGL(perturb_rank_kernel<true>, dim3((unsigned)B), dim3(PT_THREADS), (size_t)n_pow2 * 8, s, scores, (const uint8_t*)nullptr, (const int64_t*)nullptr, 1, (int)C,
                     0, descending, (int)C, n_pow2, rank, n_candidates);
  return stlt_check_launch("perturb_rank_kernel<cells>");
}

int stlt_perturb_apply_cells(const float* x, int64_t B, int64_t Cch, int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, const int32_t* rank,
                             const int32_t* n_candidates, int64_t steps, int64_t s0, int64_t s1, float fill, float* out, int32_t* removed, stlt_stream_t stream) {
  CellGeom g;
  int64_t Gt, C;
  if (const char* why = cell_geometry(B, Cch, T, H, W, ct, ch, cw, &g, &Gt, &C))
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply_cells: %s (B=%lld, x=(%lld,%lld,%lld,%lld), cells=(%lld,%lld,%lld))", why, (long long)B, (long long)Cch, (long long)T,
                          (long long)H, (long long)W, (long long)ct, (long long)ch, (long long)cw);
  if (steps < 1 || steps > 0x7fffffff || s0 < 0 || s1 < s0 || s1 > steps)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply_cells: steps >= 1 and 0 <= s0 <= s1 <= steps (got steps=%lld, s0=%lld, s1=%lld)", (long long)steps, (long long)s0,
                          (long long)s1);
  const int64_t n_steps = s1 - s0 + 1;
  if (n_steps > PT_THREADS)
    return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply_cells: %lld steps in one call (at most %d; split the range)", (long long)n_steps, PT_THREADS);
  if (B == 0) return 0;
  if (!x || !rank || !n_candidates || !out) return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply_cells: null pointer");
  const bool vec = W % 4 == 0 && cw % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int64_t items = Cch * T * H * (vec ? W / 4 : W);
  // a block re-reads the clip's C ranks, so it covers at least 4 C lane accesses; chunks * chunk >= items, below 2^32
  int64_t chunk = (int64_t)PT_THREADS * PC_ITEMS;
  if (chunk < 4 * C) chunk = (4 * C + PT_THREADS - 1) / PT_THREADS * PT_THREADS;
  const int64_t chunks = (items + chunk - 1) / chunk;
  if (chunks * B > 0x7fffffff) return stlt_set_error(STLT_EINVAL, "stlt_perturb_apply_cells: %lld workgroups in one call (at most 2^31 - 1)", (long long)(chunks * B));
  uint32_t fill_bits;
  memcpy(&fill_bits, &fill, 4);
  hipStream_t s = (hipStream_t)stream;
  StltProfScope ps(STLT_K_MISC, s);
  stlt_prof_note("perturb_apply_cells B=%lld x=(%lld,%lld,%lld,%lld) cells=%lld steps=%lld [%lld,%lld] vec=%d", (long long)B, (long long)Cch, (long long)T, (long long)H,
                 (long long)W, (long long)C, (long long)steps, (long long)s0, (long long)s1, (int)vec);
  const dim3 grid((unsigned)(chunks * B)), block(PT_THREADS);
  const size_t lds = (size_t)C * 4;
  const uint32_t* xi = reinterpret_cast<const uint32_t*>(x);
  uint32_t* oi = reinterpret_cast<uint32_t*>(out);
  if (vec)
    hipLaunchKernelGGL(perturb_apply_cells_kernel<true>, grid, block, lds, s, xi, g, (int)C, rank, n_candidates, B, steps, s0, (int)n_steps, fill_bits, (uint32_t)chunk,
                       (uint32_t)chunks, oi, removed);
  else
    hipLaunchKernelGGL(perturb_apply_cells_kernel<false>, grid, block, lds, s, xi, g, (int)C, rank, n_candidates, B, steps, s0, (int)n_steps, fill_bits, (uint32_t)chunk,
                       (uint32_t)chunks, oi, removed);
  return stlt_check_launch("perturb_apply_cells_kernel");
}

int stlt_cell_pool_abs(const float* g, int64_t B, int64_t Cch, int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, float* out, stlt_stream_t stream) {
  return cell_pool<true>("stlt_cell_pool_abs", g, B, Cch, T, H, W, ct, ch, cw, out, stream);
}

int stlt_cell_pool_sum(const float* g, int64_t B, int64_t Cch, int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, float* out, stlt_stream_t stream) {
  return cell_pool<false>("stlt_cell_pool_sum", g, B, Cch, T, H, W, ct, ch, cw, out, stream);
}

}  // extern "C"
