// Host-side fuzz of the perturbation test's entry points under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone companion of
// tests/host_fuzz.hip (same build: tests/test_host_sanitizers_perturb.py compiles the library's sources with
// `hipcc --offload-host-only -fsanitize=address,undefined -fno-gpu-sanitize`, links this driver and tests/host_fuzz_stubs.cpp; no GPU).
//
// stlt_perturb_rank, stlt_perturb_apply and stlt_perturb_curve get random, boundary and extreme extents, step ranges and pitches, null and
// misaligned FAKE device pointers: the host side never dereferences one (ASan turns that into a crash), and signed overflow in the extent /
// workgroup arithmetic trips UBSan.  Exit code 0 = no sanitizer report.
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

long g_calls = 0, g_ok = 0, g_ok_by[3] = {0, 0, 0};
void tally(int which, int rc) { ++g_calls; g_ok += rc == 0; g_ok_by[which] += rc == 0; }

void fuzz_rank() {
  void* s = nullptr;
  const int64_t B = dim(1024, 1ll << 40), T = dim(64, 1ll << 33), N = dim(36, 1ll << 33);
  tally(0, stlt_perturb_rank(F<float>(1), F<uint8_t>(2), F<int64_t>(3), B, T, N, coin(8) ? (int)uni(-2, 3) : (int)uni(0, 1), coin(8) ? (int)uni(-2, 3) : (int)uni(0, 1),
                             F<int32_t>(4), F<int32_t>(5), s));
  // the shapes the path has, up to the domain's edge: always well-formed, so that the launch arithmetic itself runs
  const int64_t Tw = uni(1, 128), Nw = uni(1, 16384 / Tw);
  tally(0, stlt_perturb_rank(FA<float>(1), FA<uint8_t>(2), FA<int64_t>(3), uni(1, 1 << 20), Tw, Nw, (int)uni(0, 1), (int)uni(0, 1), FA<int32_t>(4), FA<int32_t>(5), s));
}

void fuzz_apply() {
  void* s = nullptr;
  stlt_inputs in{};
  in.B = dim(1024, 1ll << 40);
  in.T = dim(64, 1ll << 33);
  in.N = dim(36, 1ll << 33);
  in.categories = F<int64_t>(10); in.boxes = F<float>(11); in.scores = coin(2) ? nullptr : F<float>(12);
  in.kpm_boxes = F<uint8_t>(13); in.frame_types = F<int64_t>(14); in.kpm_frames = F<uint8_t>(15); in.lengths = F<int64_t>(16);
  in.n_real_tokens = coin(2) ? 0 : (int64_t)rnd(); in.n_real_frames = coin(2) ? 0 : (int64_t)rnd();  // not read
  const int64_t steps = coin(4) ? dim(10, 1ll << 40) : uni(1, 1000);
  const int64_t s0 = coin(6) ? dim(10, 1ll << 40) : uni(0, steps > 0 ? steps : 0), s1 = coin(6) ? dim(10, 1ll << 40) : uni(s0, steps > s0 ? steps : s0);
  tally(1, stlt_perturb_apply(coin(40) ? nullptr : &in, F<int32_t>(17), F<int32_t>(18), coin(8) ? (int)uni(-2, 3) : (int)uni(0, 1), steps, s0, s1, uni(-1, 5), F<int64_t>(20),
                              F<float>(21), coin(8) ? nullptr : F<float>(22), F<uint8_t>(23), F<int64_t>(24), F<uint8_t>(25), F<int64_t>(26), F<int32_t>(27), s));
  stlt_inputs w{};
  w.B = uni(1, 4096); w.T = uni(1, 128); w.N = uni(1, 128);
  w.categories = FA<int64_t>(10); w.boxes = FA<float>(11); w.scores = coin(2) ? nullptr : FA<float>(12);
  w.kpm_boxes = FA<uint8_t>(13); w.frame_types = FA<int64_t>(14); w.kpm_frames = FA<uint8_t>(15); w.lengths = FA<int64_t>(16);
  const int64_t st = uni(1, 100000), a = uni(0, st), b = uni(a, a + 64 < st ? a + 64 : st);
  tally(1, stlt_perturb_apply(&w, FA<int32_t>(17), FA<int32_t>(18), (int)uni(0, 1), st, a, b, 3, FA<int64_t>(20), FA<float>(21), FA<float>(22), FA<uint8_t>(23), FA<int64_t>(24),
                              FA<uint8_t>(25), FA<int64_t>(26), FA<int32_t>(27), s));
}

void fuzz_curve() {
  void* s = nullptr;
  const int64_t S = dim(11, 1ll << 40), B = dim(1024, 1ll << 40), K = dim(174, 1ll << 33);
  const int64_t ld = coin(4) ? dim(174, 1ll << 40) : K + uni(0, 5);
  const bool given = coin(2);
  tally(2, stlt_perturb_curve(F<float>(30), ld, given ? F<int64_t>(31) : nullptr, coin(8) ? (int)uni(-2, 3) : (int)uni(0, 1), S, B, K, F<float>(32), F<uint8_t>(33),
                              given && coin(2) ? nullptr : F<int64_t>(34), s));
  const int64_t Kw = uni(1, 400);
  tally(2, stlt_perturb_curve(FA<float>(30), Kw + uni(0, 7), coin(2) ? FA<int64_t>(31) : nullptr, (int)uni(0, 1), uni(1, 1001), uni(1, 1 << 16), Kw, FA<float>(32), FA<uint8_t>(33),
                              FA<int64_t>(34), s));
}

}  // namespace

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 2000;
  g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
  if (stlt_version() != STLT_VERSION) { fprintf(stderr, "version mismatch\n"); return 2; }
  if (stlt_perturb_max_items() != 16384) { fprintf(stderr, "domain mismatch\n"); return 2; }
  for (long i = 0; i < iters; ++i) {
    fuzz_rank();
    fuzz_apply();
    fuzz_curve();
  }
  printf("host_fuzz_perturb: calls that returned 0: rank %ld apply %ld curve %ld\n", g_ok_by[0], g_ok_by[1], g_ok_by[2]);
  printf("host_fuzz_perturb: %ld iterations, %ld calls, %ld returned 0 (the rest refused their arguments); kernel launches configured: %ld , refused by the runtime: %ld ; last error: %s\n",
         iters, g_calls, g_ok, stlt_fake_hip_launches(), stlt_fake_hip_refused(), stlt_last_error());
  return 0;
}
