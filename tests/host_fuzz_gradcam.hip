// Host-side fuzz of the class-activation-map entry points under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone companion of
// tests/host_fuzz.hip in the style of tests/host_fuzz_ig.hip (same build: tests/test_host_sanitizers_gradcam.py compiles the library's
// sources with `hipcc --offload-host-only -fsanitize=address,undefined -fno-gpu-sanitize`, links this driver and
// tests/host_fuzz_stubs.cpp; no GPU).
//
// stlt_cam_weights (with its scratch sizing), stlt_cam_map, stlt_cam_upsample, stlt_r3d_layer_geometry and stlt_r3d_backward_layer get
// random, boundary and extreme extents, layouts and layers, null and misaligned FAKE device pointers: the host side never dereferences one
// (ASan turns that into a crash), and signed overflow in the extent / workgroup arithmetic trips UBSan.  Exit code 0 = no sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "common.h"

extern "C" long stlt_fake_hip_launches();
extern "C" long stlt_fake_hip_refused();

namespace {

uint64_t g_state = 1;
uint64_t rnd() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
int64_t uni(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }
bool coin(int one_in) { return rnd() % (uint64_t)one_in == 0; }

// a dimension: mostly the sizes the path sees, sometimes a power of two +- 1, sometimes extreme / degenerate
int64_t dim(int64_t typical_max, int64_t extreme_max) {
  switch (rnd() % 10) {
    case 0: return 0;
    case 1: return coin(2) ? -uni(1, 1000) : 1;
    case 2: { static const int64_t b[] = {16, 32, 64, 128, 16384, 65536};
              return b[rnd() % 6] + uni(-1, 1); }
    case 3: return uni(1, extreme_max);
    case 4: return extreme_max - uni(0, 3);
    default: return uni(1, typical_max);
  }
}

// Fake device memory: addresses in an unmapped range, 256-byte aligned, distinct per slot.  Never touched by a correct host path.
char* fake(int slot, int off = 0) { return (char*)(uintptr_t)(0x7e0000000000ull + (uint64_t)slot * 0x40000000ull + (uint64_t)off); }
template <typename T> T* F(int slot) { return coin(40) ? nullptr : (T*)fake(slot, coin(25) ? (int)sizeof(T) : 0); }
template <typename T> T* FA(int slot) { return (T*)fake(slot); }

long g_calls = 0, g_ok = 0, g_ok_by[5] = {0, 0, 0, 0, 0};
void tally(int which, int rc) { ++g_calls; g_ok += rc == 0; g_ok_by[which] += rc == 0; }

int layout_any() { return coin(8) ? (int)uni(-2, 5) : (int)uni(0, 1); }

void fuzz_weights() {
  void* s = nullptr;
  const int64_t B = dim(64, 1ll << 40), P = dim(12544, 1ll << 40), C = dim(2048, 1ll << 40);
  const size_t need = stlt_cam_scratch_bytes(B, P, C);
  tally(0, stlt_cam_weights(F<float>(10), B, P, C, layout_any(), F<float>(11), coin(10) ? nullptr : (void*)fake(12, coin(20) ? 4 : 0),
                            coin(6) ? (size_t)rnd() % (need + 64) : need, s));
  // well-formed, both layouts, every misalignment of g by a multiple of 4 bytes, channel counts around the vector width and the wave
  const int64_t Bw = uni(1, 64), Pw = uni(1, 4096), Cw = coin(2) ? uni(1, 300) : 4 * uni(1, 512);
  tally(0, stlt_cam_weights((float*)fake(10, 4 * (int)uni(0, 3)), Bw, Pw, Cw, (int)uni(0, 1), (float*)fake(11, 4 * (int)uni(0, 3)), (void*)fake(12),
                            stlt_cam_scratch_bytes(Bw, Pw, Cw), s));
}

void fuzz_map() {
  void* s = nullptr;
  tally(1, stlt_cam_map(F<float>(20), F<float>(21), (int)uni(-1, 2), dim(64, 1ll << 40), dim(12544, 1ll << 40), dim(2048, 1ll << 40), layout_any(), (int)uni(-1, 2),
                        F<float>(22), s));
  const int64_t Cw = coin(2) ? uni(1, 300) : 4 * uni(1, 512);
  tally(1, stlt_cam_map((float*)fake(20, 4 * (int)uni(0, 3)), (float*)fake(21, 4 * (int)uni(0, 3)), (int)uni(0, 1), uni(1, 64), uni(1, 4096), Cw, (int)uni(0, 1),
                        (int)uni(0, 1), (float*)fake(22, 4 * (int)uni(0, 3)), s));
}

void fuzz_upsample() {
  void* s = nullptr;
  tally(2, stlt_cam_upsample(F<float>(30), dim(64, 1ll << 40), dim(4, 1ll << 33), dim(7, 1ll << 33), dim(7, 1ll << 33), dim(32, 1ll << 33), dim(224, 1ll << 33),
                             dim(224, 1ll << 33), F<float>(31), s));
  tally(2, stlt_cam_upsample(FA<float>(30), uni(1, 16), uni(1, 16), uni(1, 28), uni(1, 28), uni(1, 32), uni(1, 224), uni(1, 224), FA<float>(31), s));
}

void fuzz_geometry() {
  const bool wild = coin(4);
  const int64_t B = wild ? dim(4, 1ll << 21) : uni(1, 64), T = wild ? dim(16, 4100) : uni(1, 33), H = wild ? dim(112, 4100) : uni(1, 230),
                W = wild ? dim(112, 4100) : uni(1, 230);
  int64_t dims[4] = {-1, -1, -1, -1};
  size_t off = 0;
  const int layer = coin(6) ? (int)uni(-2, 7) : (int)uni(1, 4);
  const bool no_dims = coin(30), no_off = coin(30);
  const int rc = stlt_r3d_layer_geometry(B, T, H, W, layer, no_dims ? nullptr : dims, no_off ? nullptr : &off);
  tally(3, rc);
  const size_t tape = stlt_r3d_tape_bytes(B, T, H, W);
  if (rc == 0) {  // inside the tape, on 256 bytes, with positive extents
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || dims[3] < 1 || (off & 255) || off + (size_t)(B * dims[0] * dims[1] * dims[2] * dims[3]) * 4 > tape) {
      fprintf(stderr, "stlt_r3d_layer_geometry: a slot outside the tape\n");
      exit(3);
    }
  } else if (layer >= 1 && layer <= 4 && tape != 0 && !no_dims && !no_off) {  // it fails for exactly the shapes the tape query returns 0 for
    fprintf(stderr, "stlt_r3d_layer_geometry refused a shape the tape accepts: %s\n", stlt_last_error());
    exit(3);
  }
}

void fuzz_backward_layer() {
  void* s = nullptr;
  const bool wild = coin(5);
  const int64_t B = wild ? dim(4, 1ll << 21) : uni(1, 4), T = wild ? dim(16, 4100) : uni(1, 33), H = wild ? dim(112, 4100) : uni(1, 130),
                W = wild ? dim(112, 4100) : uni(1, 130);
  const bool tidy = !coin(3);
  stlt_r3d_params p;
  float* dg[STLT_R3D_CONVS];
  for (int i = 0; i < STLT_R3D_CONVS; ++i) {
    auto ptr = [&](int slot) { return tidy ? FA<float>(slot) : F<float>(slot); };
    p.conv[i] = stlt_r3d_conv{ptr(400 + i), ptr(460), ptr(461), ptr(462), ptr(463)};
    dg[i] = ptr(530 + i);
  }
  p.bn_eps = 1e-5f;
  if (coin(3)) dg[0] = nullptr;  // the stem's thin copy is not read
  const size_t tape = stlt_r3d_tape_bytes(B, T, H, W), bws = stlt_r3d_backward_workspace_bytes(B, T, H, W);
  const float* dfeat = coin(2) ? FA<float>(655) : nullptr;
  const float* dpool = dfeat ? nullptr : FA<float>(656);
  if (!tidy && coin(4)) { dfeat = coin(2) ? FA<float>(655) : nullptr; dpool = dfeat ? FA<float>(656) : nullptr; }
  const int layer = tidy ? (int)uni(1, 3) : (int)uni(-1, 5);
  float* dlayer = tidy ? FA<float>(660) : (coin(6) ? nullptr : (float*)fake(660, coin(4) ? 4 * (int)uni(1, 3) : 0));
  tally(4, stlt_r3d_backward_layer(!tidy && coin(10) ? nullptr : &p, !tidy && coin(10) ? nullptr : dg, tidy || !coin(10) ? (void*)fake(654) : nullptr,
                                   !tidy && coin(6) ? (size_t)rnd() % (tape + 64) : tape, B, T, H, W, dfeat, dpool, layer, dlayer,
                                   tidy || !coin(10) ? (void*)fake(657, !tidy && coin(10) ? 16 : 0) : nullptr, !tidy && coin(6) ? (size_t)rnd() % (bws + 64) : bws, s));
}

}  // namespace

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 2000;
  g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
  if (stlt_version() != STLT_VERSION) { fprintf(stderr, "version mismatch\n"); return 2; }
  if (stlt_cam_scratch_bytes(1, STLT_CAM_CHUNK + 1, 1) != 8 || stlt_cam_scratch_bytes(1, STLT_CAM_CHUNK, 1) != 0) { fprintf(stderr, "chunk mismatch\n"); return 2; }
  for (long i = 0; i < iters; ++i) {
    fuzz_weights();
    fuzz_map();
    fuzz_upsample();
    fuzz_geometry();
    fuzz_backward_layer();
  }
  printf("host_fuzz_gradcam: calls that returned 0: weights %ld map %ld upsample %ld geometry %ld backward_layer %ld\n", g_ok_by[0], g_ok_by[1], g_ok_by[2], g_ok_by[3],
         g_ok_by[4]);
  printf("host_fuzz_gradcam: %ld iterations, %ld calls, %ld returned 0 (the rest refused their arguments); kernel launches configured: %ld , refused by the runtime: %ld ; last error: %s\n",
         iters, g_calls, g_ok, stlt_fake_hip_launches(), stlt_fake_hip_refused(), stlt_last_error());
  return 0;
}
