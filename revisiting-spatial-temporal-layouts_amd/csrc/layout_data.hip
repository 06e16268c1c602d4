// Device layout dataset (layout_data.py): the per-video half of the reference's StltDataset.__getitem__
// (src/modelling/datasets.py:52-125) and its StltCollater (datasets.py:239-288) over tables uploaded once.
//   layout_boxes_kernel  — fix_box (src/utils/data_utils.py:205-231) + `torch.tensor(box) / video_size` for every kept object, once;
//   layout_batch_kernel  — one launch per batch: the padded batch, both key-padding masks, lengths and labels.
// Both kernels are element-wise and memory-bound: 256 threads per workgroup, at most 2048 workgroups, grid-stride loops.
#include "common.h"

namespace {

constexpr int LD_THREADS = 256;
constexpr int64_t LD_MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups (cdna_hip_programming.md, Guideline 11)

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

unsigned ld_grid(int64_t work) {
  const int64_t blocks = (work + LD_THREADS - 1) / LD_THREADS;
  return (unsigned)(blocks < LD_MAX_BLOCKS ? blocks : LD_MAX_BLOCKS);
}

// raw: (K, 4) int32 = max(0, int(b)) saturated at 2^30; size: (K, 2) int32 = the object's video (w, h); out: (K, 4) float32
__global__ __launch_bounds__(LD_THREADS) void layout_boxes_kernel(const i32x4* __restrict__ raw, const i32x2* __restrict__ size, int64_t K,
                                                                  f32x4* __restrict__ out) {
  for (int64_t k = (int64_t)blockIdx.x * LD_THREADS + threadIdx.x; k < K; k += (int64_t)gridDim.x * LD_THREADS) {
    const i32x4 r = raw[k];
    const i32x2 wh = size[k];
    const int w = wh.x, h = wh.y;
    int b0 = r.x, b1 = r.y, b2 = r.z, b3 = r.w;  // fix_box, statement by statement (the max(0, .) is already applied)
    if (b0 > b2) { const int t = b0; b0 = b2; b2 = t; }
    if (b1 > b3) { const int t = b1; b1 = b3; b3 = t; }
    if (b0 >= w) b0 = w - 1;
    if (b1 >= h) b1 = h - 1;
    if (b2 >= w) b2 = w - 1;
    if (b3 >= h) b3 = h - 1;
    if (b0 == b2 && b0 == 0) b2 = 1;
    if (b1 == b3 && b1 == 0) b3 = 1;
    if (b0 == b2) b0 -= 1;
    if (b1 == b3) b1 -= 1;
    // int64 / int64 true division: both sides in float32 (exact below 2^24), one correctly rounded division each
    const float fw = (float)w, fh = (float)h;
    out[k] = f32x4{(float)b0 / fw, (float)b1 / fh, (float)b2 / fw, (float)b3 / fh};
  }
}

// One item per (clip, frame, slot) of the padded batch, then one per (clip, label column).  `packed` = video index (B), sampled
// frame count (B), then the sampled frame indices (B x T, row b's first count[b] entries used).
__global__ __launch_bounds__(LD_THREADS) void layout_batch_kernel(stlt_layout_table tab, const int32_t* __restrict__ packed, int64_t B, int T,
                                                                  int Lf, int N, int64_t* __restrict__ cat, f32x4* __restrict__ box,
                                                                  float* __restrict__ score, int64_t* __restrict__ ft,
                                                                  uint8_t* __restrict__ kpm_boxes, uint8_t* __restrict__ kpm_frames,
                                                                  int64_t* __restrict__ lengths, void* __restrict__ labels) {
  const int64_t n_slots = B * Lf * N;
  const int64_t n_cols = tab.n_classes > 0 ? tab.n_classes : 1;
  const int64_t total = n_slots + B * n_cols;
  const int32_t* vid = packed;
  const int32_t* cnt = packed + B;
  const int32_t* fidx = packed + 2 * B;
  for (int64_t i = (int64_t)blockIdx.x * LD_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * LD_THREADS) {
    if (i < n_slots) {
      const int n = (int)(i % N);
      const int64_t bt = i / N;
      const int t = (int)(bt % Lf);
      const int64_t b = bt / Lf;
      const int ns = cnt[b];
      // extract frame (datasets.py:97-113) and pad frames (datasets.py:247-270) hold the CLS object alone
      int64_t c = n == 0 ? tab.cls_id : 0;
      f32x4 bx = n == 0 ? f32x4{0.f, 0.f, 1.f, 1.f} : f32x4{0.f, 0.f, 0.f, 0.f};
      float sc = n == 0 ? 1.f : 0.f;
      int64_t type = t == ns ? tab.type_extract : 0;  // frame2type["pad"] = 0 (configs.py:79-89)
      if (t < ns) {  // a sampled frame: CLS, its kept objects in file order, zero slots (datasets.py:63-94)
        const int64_t gf = tab.video_frames[vid[b]] + fidx[b * T + t];
        const int64_t o0 = tab.frame_objects[gf];
        const int64_t k = tab.frame_objects[gf + 1] - o0;
        if (n >= 1 && n <= k) {
          const int64_t o = o0 + n - 1;
          c = tab.object_category[o];
          bx = reinterpret_cast<const f32x4*>(tab.object_box)[o];
          sc = tab.object_score[o];
        }
        type = tab.frame_empty[gf] ? tab.type_empty : tab.type_regular;
      }
      cat[i] = c;
      box[i] = bx;
      if (score) score[i] = sc;
      kpm_boxes[i] = c == 0;  // categories == 0 (datasets.py:274-278)
      if (n == 0) {
        ft[bt] = type;
        kpm_frames[bt] = type == 0;  // frame_types == pad (datasets.py:280-286)
      }
    } else {
      const int64_t j = i - n_slots;
      const int64_t b = j / n_cols, col = j % n_cols;
      const int32_t v = vid[b];
      if (col == 0) lengths[b] = (int64_t)cnt[b] + 1;
      if (tab.n_classes > 0) {  // multi-hot of int(action[1:]) (datasets.py:133-136)
        float hot = 0.f;
        for (int64_t a = tab.video_actions[v]; a < tab.video_actions[v + 1]; ++a) hot = tab.actions[a] == col ? 1.f : hot;
        static_cast<float*>(labels)[b * n_cols + col] = hot;
      } else {
        static_cast<int64_t*>(labels)[b] = tab.video_label[v];
      }
    }
  }
}

bool ld_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int stlt_layout_boxes_fwd(const int32_t* raw_boxes, const int32_t* sizes, int64_t n_objects, float* boxes, stlt_stream_t stream) {
  if (n_objects < 0 || n_objects > ((int64_t)1 << 40)) return stlt_set_error(STLT_EINVAL, "stlt_layout_boxes_fwd: bad object count %lld", (long long)n_objects);
  if (n_objects == 0) return 0;
  if (!raw_boxes || !sizes || !boxes) return stlt_set_error(STLT_EINVAL, "stlt_layout_boxes_fwd: null pointer");
  if (ld_misaligned(raw_boxes, 16) || ld_misaligned(boxes, 16) || ld_misaligned(sizes, 8))
    return stlt_set_error(STLT_EINVAL, "stlt_layout_boxes_fwd: raw_boxes / boxes need 16-byte, sizes 8-byte alignment");
  hipLaunchKernelGGL(layout_boxes_kernel, dim3(ld_grid(n_objects)), dim3(LD_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const i32x4*>(raw_boxes), reinterpret_cast<const i32x2*>(sizes), n_objects, reinterpret_cast<f32x4*>(boxes));
  return stlt_check_launch("layout_boxes_kernel");
}

extern "C" int stlt_layout_batch_fwd(const stlt_layout_table* table, const int32_t* batch_host, int32_t* batch_dev, int64_t B, int64_t T,
                                     int64_t L, int64_t N, int64_t* categories, float* boxes, float* scores, int64_t* frame_types,
                                     uint8_t* kpm_boxes, uint8_t* kpm_frames, int64_t* lengths, void* labels, stlt_stream_t stream) {
  if (!table || !batch_host || !batch_dev || !categories || !boxes || !frame_types || !kpm_boxes || !kpm_frames || !lengths || !labels)
    return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: null pointer");
  const stlt_layout_table& tb = *table;
  if (B <= 0 || T <= 0 || L <= 0 || N <= 0 || B > (1 << 24) || T > (1 << 16) || L > T + 1 || N > (1 << 16))
    return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: bad shape B=%lld T=%lld L=%lld N=%lld", (long long)B, (long long)T, (long long)L,
                          (long long)N);
  if (tb.n_videos <= 0 || tb.n_frames < 0 || tb.n_objects < 0 || tb.n_actions < 0 || tb.n_classes < 0 || tb.n_videos > INT32_MAX ||
      tb.n_classes > (1 << 24) || !tb.video_frames_host || !tb.frame_objects_host || !tb.video_frames || !tb.frame_objects ||
      !tb.frame_empty || !tb.object_category || !tb.object_score || !tb.object_box)
    return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: bad table");
  if (tb.n_classes > 0 ? (!tb.video_actions_host || !tb.actions_host || !tb.video_actions || !tb.actions) : !tb.video_label)
    return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: table lacks its label arrays");
  if (ld_misaligned(boxes, 16) || ld_misaligned(tb.object_box, 16))
    return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: boxes need 16-byte alignment");
  const int32_t* vid = batch_host;
  const int32_t* cnt = batch_host + B;
  const int32_t* fidx = batch_host + 2 * B;
  int64_t max_len = 0;
  for (int64_t b = 0; b < B; ++b) {  // everything the kernel will index, checked before the copy and the launch
    const int64_t v = vid[b], ns = cnt[b];
    if (v < 0 || v >= tb.n_videos) return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: clip %lld: video %lld out of range", (long long)b, (long long)v);
    const int64_t f0 = tb.video_frames_host[v], f1 = tb.video_frames_host[v + 1];
    if (f0 < 0 || f1 < f0 || f1 > tb.n_frames) return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: video %lld: bad frame offsets", (long long)v);
    if (ns < 0 || ns > T) return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: clip %lld: %lld sampled frames, T = %lld", (long long)b, (long long)ns, (long long)T);
    if (ns + 1 > max_len) max_len = ns + 1;
    for (int64_t t = 0; t < ns; ++t) {
      const int64_t f = fidx[b * T + t];
      if (f < 0 || f >= f1 - f0)
        return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: clip %lld: frame index %lld outside the video's %lld frames", (long long)b, (long long)f,
                              (long long)(f1 - f0));
      const int64_t o0 = tb.frame_objects_host[f0 + f], o1 = tb.frame_objects_host[f0 + f + 1];
      if (o0 < 0 || o1 < o0 || o1 > tb.n_objects || o1 - o0 > N - 1)
        return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: frame %lld: bad object offsets for N = %lld", (long long)(f0 + f), (long long)N);
    }
    if (tb.n_classes > 0) {
      const int64_t a0 = tb.video_actions_host[v], a1 = tb.video_actions_host[v + 1];
      if (a0 < 0 || a1 < a0 || a1 > tb.n_actions) return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: video %lld: bad action offsets", (long long)v);
      for (int64_t a = a0; a < a1; ++a)
        if (tb.actions_host[a] < 0 || tb.actions_host[a] >= tb.n_classes)
          return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: video %lld: action %d out of range", (long long)v, tb.actions_host[a]);
    }
  }
  if (max_len > L) return stlt_set_error(STLT_EINVAL, "stlt_layout_batch_fwd: L = %lld below the longest clip (%lld)", (long long)L, (long long)max_len);
  hipStream_t s = (hipStream_t)stream;
  if (hipError_t e = hipMemcpyAsync(batch_dev, batch_host, (size_t)B * (size_t)(2 + T) * sizeof(int32_t), hipMemcpyHostToDevice, s); e != hipSuccess)
    return stlt_set_error((int)e, "stlt_layout_batch_fwd: index copy: %s", hipGetErrorString(e));
  const int64_t work = B * L * N + B * (tb.n_classes > 0 ? tb.n_classes : 1);
  hipLaunchKernelGGL(layout_batch_kernel, dim3(ld_grid(work)), dim3(LD_THREADS), 0, s, tb, batch_dev, B, (int)T, (int)L, (int)N, categories,
                     reinterpret_cast<f32x4*>(boxes), scores, frame_types, kpm_boxes, kpm_frames, lengths, labels);
  return stlt_check_launch("layout_batch_kernel");
}
