// Host-side fuzz of the integrated-gradients entry points under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone companion of
// tests/host_fuzz.hip in the style of tests/host_fuzz_perturb.hip (same build: tests/test_host_sanitizers_ig.py compiles the library's
// sources with `hipcc --offload-host-only -fsanitize=address,undefined -fno-gpu-sanitize`, links this driver and
// tests/host_fuzz_stubs.cpp; no GPU).
//
// stlt_ig_path, stlt_ig_path_dense, stlt_ig_reduce, stlt_ig_delta (with its scratch sizing) and stlt_cell_pool_sum get random, boundary
// and extreme extents, step ranges, flags and group sizes, null and misaligned FAKE device pointers: the host side never dereferences one
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

// a step range: mostly well-formed, sometimes anything
void steps_range(int64_t* steps, int64_t* s0, int64_t* s1) {
  *steps = coin(4) ? dim(16, 1ll << 40) : uni(1, 1000);
  *s0 = coin(6) ? dim(10, 1ll << 40) : uni(0, *steps > 0 ? *steps : 0);
  *s1 = coin(6) ? dim(10, 1ll << 40) : uni(*s0, *steps > *s0 ? (*s0 + 255 < *steps ? *s0 + 255 : *steps) : *s0);
}

void fuzz_path() {
  void* s = nullptr;
  stlt_inputs in{};
  in.B = dim(1024, 1ll << 40);
  in.T = dim(64, 1ll << 33);
  in.N = dim(36, 1ll << 33);
  in.categories = F<int64_t>(10); in.boxes = F<float>(11); in.scores = coin(2) ? nullptr : F<float>(12);
  in.kpm_boxes = F<uint8_t>(13); in.frame_types = F<int64_t>(14); in.kpm_frames = F<uint8_t>(15); in.lengths = F<int64_t>(16);
  in.n_real_tokens = coin(2) ? 0 : (int64_t)rnd(); in.n_real_frames = coin(2) ? 0 : (int64_t)rnd();  // not read
  int64_t steps, s0, s1;
  steps_range(&steps, &s0, &s1);
  tally(0, stlt_ig_path(coin(40) ? nullptr : &in, coin(2) ? nullptr : F<float>(17), coin(2) ? nullptr : F<float>(18), steps, s0, s1, F<int64_t>(20), F<float>(21),
                        coin(8) ? nullptr : F<float>(22), F<uint8_t>(23), F<int64_t>(24), F<uint8_t>(25), F<int64_t>(26), s));
  stlt_inputs w{};
  w.B = uni(1, 4096); w.T = uni(1, 128); w.N = uni(1, 128);
  w.categories = FA<int64_t>(10); w.boxes = FA<float>(11); w.scores = coin(2) ? nullptr : FA<float>(12);
  w.kpm_boxes = FA<uint8_t>(13); w.frame_types = FA<int64_t>(14); w.kpm_frames = FA<uint8_t>(15); w.lengths = FA<int64_t>(16);
  const int64_t st = uni(1, 100000), a = uni(0, st), b = uni(a, a + 64 < st ? a + 64 : st);
  tally(0, stlt_ig_path(&w, coin(2) ? nullptr : FA<float>(17), coin(2) ? nullptr : FA<float>(18), st, a, b, FA<int64_t>(20), FA<float>(21), FA<float>(22), FA<uint8_t>(23),
                        FA<int64_t>(24), FA<uint8_t>(25), FA<int64_t>(26), s));
}

void fuzz_dense() {
  void* s = nullptr;
  int64_t steps, s0, s1;
  steps_range(&steps, &s0, &s1);
  const float fill = coin(2) ? 0.f : (float)uni(-3, 3);
  tally(1, stlt_ig_path_dense(F<float>(30), coin(2) ? nullptr : F<float>(31), fill, dim(64, 1ll << 40), dim(602112, 1ll << 40), steps, s0, s1, F<float>(32), s));
  // well-formed, every combination of pointer misalignments (a multiple of 4 bytes) and element counts around the vector width
  const int64_t st = uni(1, 100000), a = uni(0, st), b = uni(a, a + 255 < st ? a + 255 : st);
  tally(1, stlt_ig_path_dense((float*)fake(30, 4 * (int)uni(0, 3)), coin(2) ? nullptr : (float*)fake(31, 4 * (int)uni(0, 3)), fill, uni(1, 64), uni(1, 1 << 20), st, a, b,
                              (float*)fake(32, 4 * (int)uni(0, 3)), s));
}

void fuzz_reduce() {
  void* s = nullptr;
  int64_t steps, s0, s1;
  steps_range(&steps, &s0, &s1);
  const int flags = coin(8) ? (int)uni(-2, 9) : (int)uni(0, 3);
  const bool want_group = coin(3);
  tally(2, stlt_ig_reduce(F<float>(40), dim(64, 1ll << 40), dim(602112, 1ll << 40), steps, s0, s1, flags, F<float>(41), coin(3) ? nullptr : F<float>(42),
                          coin(2) ? nullptr : F<float>(43), 0.f, coin(3) ? nullptr : F<float>(44), want_group ? dim(4, 1ll << 40) : 1, coin(3) ? F<float>(45) : nullptr,
                          want_group ? F<float>(46) : nullptr, s));
  const int64_t st = uni(1, 100000), a = uni(0, st), b = uni(a, a + 255 < st ? a + 255 : st), group = uni(1, 8), n = group * uni(1, 1 << 16);
  const bool fin = coin(2), grp = fin && coin(2);
  tally(2, stlt_ig_reduce(FA<float>(40), uni(1, 64), n, st, a, b, (coin(2) ? STLT_IG_BEGIN : 0) | (fin ? STLT_IG_FINISH : 0), FA<float>(41), FA<float>(42),
                          coin(2) ? nullptr : FA<float>(43), 0.f, FA<float>(44), grp ? group : 1, grp && coin(2) ? FA<float>(45) : nullptr, grp ? FA<float>(46) : nullptr, s));
}

void fuzz_delta() {
  void* s = nullptr;
  const int64_t B = dim(64, 1ll << 40), n0 = dim(8192, 1ll << 40), n1 = coin(2) ? 0 : dim(8192, 1ll << 40), n2 = coin(2) ? 0 : dim(602112, 1ll << 40);
  const size_t need = stlt_ig_delta_scratch_bytes(B, n0, n1, n2);
  tally(3, stlt_ig_delta(F<float>(50), n0, F<float>(51), n1, F<float>(52), n2, F<float>(53), F<float>(54), F<float>(55), B, dim(174, 1ll << 40), coin(4) ? dim(64, 1ll << 40) : 0,
                         coin(20) ? nullptr : (void*)fake(56, coin(25) ? 2 : 0), coin(6) ? (size_t)rnd() % (need + 64) : need, F<float>(57), s));
  const int64_t Bw = uni(1, 64), m0 = uni(1, 1 << 20), m1 = coin(2) ? 0 : uni(1, 1 << 12), m2 = coin(2) ? 0 : uni(1, 1 << 20);
  tally(3, stlt_ig_delta(FA<float>(50), m0, FA<float>(51), m1, FA<float>(52), m2, FA<float>(53), FA<float>(54), FA<float>(55), Bw, uni(1, 400), coin(2) ? uni(1, 4096) : 0,
                         (void*)fake(56), stlt_ig_delta_scratch_bytes(Bw, m0, m1, m2), FA<float>(57), s));
}

void fuzz_pool() {
  void* s = nullptr;
  tally(4, stlt_cell_pool_sum(F<float>(60), dim(64, 1ll << 40), dim(3, 1ll << 33), dim(16, 1ll << 33), dim(112, 1ll << 33), dim(112, 1ll << 33), dim(16, 1ll << 33),
                              dim(32, 1ll << 33), dim(32, 1ll << 33), F<float>(61), s));
  tally(4, stlt_cell_pool_sum(FA<float>(60), uni(1, 64), uni(1, 4), uni(1, 32), uni(1, 128), uni(1, 128), uni(4, 16), uni(8, 32), uni(8, 32), FA<float>(61), s));
}

}  // namespace

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 2000;
  g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
  if (stlt_version() != STLT_VERSION) { fprintf(stderr, "version mismatch\n"); return 2; }
  if (stlt_ig_delta_scratch_bytes(1, STLT_IG_DELTA_CHUNK + 1, 0, 0) != 8) { fprintf(stderr, "chunk mismatch\n"); return 2; }
  for (long i = 0; i < iters; ++i) {
    fuzz_path();
    fuzz_dense();
    fuzz_reduce();
    fuzz_delta();
    fuzz_pool();
  }
  printf("host_fuzz_ig: calls that returned 0: path %ld dense %ld reduce %ld delta %ld pool %ld\n", g_ok_by[0], g_ok_by[1], g_ok_by[2], g_ok_by[3], g_ok_by[4]);
  printf("host_fuzz_ig: %ld iterations, %ld calls, %ld returned 0 (the rest refused their arguments); kernel launches configured: %ld , refused by the runtime: %ld ; last error: %s\n",
         iters, g_calls, g_ok, stlt_fake_hip_launches(), stlt_fake_hip_refused(), stlt_last_error());
  return 0;
}
