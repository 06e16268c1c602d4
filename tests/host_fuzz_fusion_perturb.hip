// Host-side fuzz of the appearance side of the perturbation test under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone companion
// of tests/host_fuzz_perturb.hip (same build: tests/test_host_sanitizers_fusion_perturb.py compiles the library's sources with
// `hipcc --offload-host-only -fsanitize=address,undefined -fno-gpu-sanitize`, links this driver and tests/host_fuzz_stubs.cpp; no GPU).
//
// stlt_perturb_rank_cells, stlt_perturb_apply_cells and stlt_cell_pool_abs get random, boundary and extreme extents, cell sizes and step
// ranges, null and misaligned FAKE device pointers: the host side never dereferences one (ASan turns that into a crash), and signed overflow
// in the extent / grid / workgroup arithmetic trips UBSan.  Exit code 0 = no sanitizer report.
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
template <typename T> T* F(int slot) { return coin(40) ? nullptr : (T*)fake(slot, coin(4) ? (int)sizeof(T) * (int)uni(1, 3) : 0); }
template <typename T> T* FA(int slot) { return (T*)fake(slot); }

long g_calls = 0, g_ok = 0, g_ok_by[3] = {0, 0, 0};
void tally(int which, int rc) { ++g_calls; g_ok += rc == 0; g_ok_by[which] += rc == 0; }

void fuzz_rank_cells() {
  void* s = nullptr;
  tally(0, stlt_perturb_rank_cells(F<float>(1), dim(1024, 1ll << 40), dim(64, 1ll << 33), coin(8) ? (int)uni(-2, 3) : (int)uni(0, 1), F<int32_t>(2), F<int32_t>(3), s));
  // the shapes the path has, up to the domain's edge: always well-formed, so that the launch arithmetic itself runs
  tally(0, stlt_perturb_rank_cells(FA<float>(1), uni(1, 1 << 20), coin(6) ? 16384 - uni(0, 2) : uni(1, 16384), (int)uni(0, 1), FA<int32_t>(2), FA<int32_t>(3), s));
}

void fuzz_apply_cells() {
  void* s = nullptr;
  const int64_t steps = coin(4) ? dim(10, 1ll << 40) : uni(1, 1000);
  const int64_t s0 = coin(6) ? dim(10, 1ll << 40) : uni(0, steps > 0 ? steps : 0), s1 = coin(6) ? dim(10, 1ll << 40) : uni(s0, steps > s0 ? steps : s0);
  const float fill = coin(3) ? 0.f : (float)uni(-3, 3) * 0.5f;
  tally(1, stlt_perturb_apply_cells(F<float>(10), dim(64, 1ll << 40), dim(3, 1ll << 33), dim(32, 1ll << 33), dim(112, 1ll << 33), dim(112, 1ll << 33), dim(16, 1ll << 33),
                                    dim(32, 1ll << 33), dim(32, 1ll << 33), F<int32_t>(11), F<int32_t>(12), steps, s0, s1, fill, F<float>(13), coin(3) ? nullptr : F<int32_t>(14), s));
  // well-formed: a video cut by the trunk's strides, or a feature map cut into columns, any alignment of x and out
  const bool video = coin(2);
  const int64_t Cch = video ? 3 : uni(1, 2048), T = video ? uni(1, 64) : uni(1, 4), H = video ? uni(1, 256) : uni(1, 8), W = video ? uni(1, 256) : uni(1, 8);
  const int64_t ct = video ? 16 : 1, ch = video ? 32 : 1, cw = video ? (coin(4) ? uni(1, 40) : 32) : 1;
  const int64_t st = uni(1, 100000), a = uni(0, st), b = uni(a, a + 64 < st ? a + 64 : st);
  tally(1, stlt_perturb_apply_cells((const float*)fake(10, 4 * (int)uni(0, 4)), uni(1, 4096), Cch, T, H, W, ct, ch, cw, FA<int32_t>(11), FA<int32_t>(12), st, a, b, fill,
                                    (float*)fake(13, 4 * (int)uni(0, 4)), coin(2) ? nullptr : FA<int32_t>(14), s));
  // the edges of the domain: a clip just below 2^31 elements, a grid of exactly 16384 cells and one beyond
  if (coin(8)) {
    tally(1, stlt_perturb_apply_cells(FA<float>(10), uni(1, 2), 1, 1, 1 << 15, (1 << 16) - uni(0, 1), 1, 1 << 8, (1 << 9) - uni(0, 1), FA<int32_t>(11), FA<int32_t>(12), 10, 0, 10,
                                      fill, FA<float>(13), nullptr, s));
    tally(1, stlt_perturb_apply_cells(FA<float>(10), 1, 2, 4, 64, 64 + uni(0, 1), 1, 1, 1, FA<int32_t>(11), FA<int32_t>(12), 10, 3, 7, fill, FA<float>(13), FA<int32_t>(14), s));
  }
}

void fuzz_pool() {
  void* s = nullptr;
  tally(2, stlt_cell_pool_abs(F<float>(20), dim(64, 1ll << 40), dim(3, 1ll << 33), dim(32, 1ll << 33), dim(112, 1ll << 33), dim(112, 1ll << 33), dim(16, 1ll << 33), dim(32, 1ll << 33),
                              dim(32, 1ll << 33), F<float>(21), s));
  const bool video = coin(2);
  tally(2, stlt_cell_pool_abs(FA<float>(20), uni(1, 4096), video ? 3 : uni(1, 2048), video ? uni(1, 64) : uni(1, 4), video ? uni(1, 256) : uni(1, 8), video ? uni(1, 256) : uni(1, 8),
                              video ? 16 : 1, video ? 32 : 1, video ? 32 : 1, FA<float>(21), s));
}

}  // namespace

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 2000;
  g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
  if (stlt_version() != STLT_VERSION) { fprintf(stderr, "version mismatch\n"); return 2; }
  if (stlt_perturb_max_items() != 16384) { fprintf(stderr, "domain mismatch\n"); return 2; }
  for (long i = 0; i < iters; ++i) {
    fuzz_rank_cells();
    fuzz_apply_cells();
    fuzz_pool();
  }
  printf("host_fuzz_fusion_perturb: calls that returned 0: rank_cells %ld apply_cells %ld pool %ld\n", g_ok_by[0], g_ok_by[1], g_ok_by[2]);
  printf("host_fuzz_fusion_perturb: %ld iterations, %ld calls, %ld returned 0 (the rest refused their arguments); kernel launches configured: %ld , refused by the runtime: %ld ; last error: %s\n",
         iters, g_calls, g_ok, stlt_fake_hip_launches(), stlt_fake_hip_refused(), stlt_last_error());
  return 0;
}
