// Host-side fuzz of the fusion models' relevance entry points under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
// companion of tests/host_fuzz.hip (same build: tests/test_host_sanitizers_fusion_relevance.py compiles the library's sources with
// `hipcc --offload-host-only -fsanitize=address,undefined -fno-gpu-sanitize`, links this driver and tests/host_fuzz_stubs.cpp; no GPU).
//
// stlt_attn_grad_probs_cross, stlt_attn_rollout_joint, stlt_relevance_combine_joint, stlt_attn_block_bwd_relevance and
// stlt_train_backward_relevance with STLT_FLAG_TRAIN_BACKBONE get random, boundary and extreme shapes, null and misaligned FAKE device
// pointers: the host side never dereferences one (ASan turns that into a crash), and signed overflow in the unit / workgroup arithmetic
// trips UBSan.  Exit code 0 = no sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>
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

// a dimension: mostly the sizes the path sees, sometimes a tile boundary +- 1, sometimes extreme / degenerate
int64_t dim(int64_t typical_max, int64_t extreme_max) {
  switch (rnd() % 10) {
    case 0: return 0;
    case 1: return coin(2) ? -uni(1, 1000) : 1;
    case 2: { static const int64_t b[] = {16, 32, 48, 64, 128, 256};
              return b[rnd() % 6] + uni(-1, 1); }
    case 3: return uni(1, extreme_max);
    case 4: return extreme_max - uni(0, 3);
    default: return uni(1, typical_max);
  }
}

// Fake device memory: addresses in an unmapped range, 256-byte aligned, distinct per slot.  Never touched by a correct host path.
char* fake(int slot, int off = 0) { return (char*)(uintptr_t)(0x7e0000000000ull + (uint64_t)slot * 0x40000000ull + (uint64_t)off); }
template <typename T> T* F(int slot) { return coin(40) ? nullptr : (T*)fake(slot, coin(25) ? (coin(2) ? 4 : 2) : 0); }
template <typename T> T* FA(int slot) { return (T*)fake(slot); }

long g_calls = 0, g_ok = 0, g_ok_by[5] = {0, 0, 0, 0, 0};
void tally(int which, int rc) { ++g_calls; g_ok += rc == 0; g_ok_by[which] += rc == 0; }

void fuzz_ops() {
  void* s = nullptr;
  const int64_t S = dim(2048, 1ll << 31), Lq = dim(64, 300), Lk = coin(3) ? Lq : dim(64, 300), H = dim(12, 70000);
  const int64_t dh = coin(2) ? 64 : dim(64, 300), d = H > 0 && dh > 0 && H < 4096 ? H * dh : 64;
  const int64_t ldq = coin(6) ? dim(3072, 1ll << 32) : d * uni(1, 3), ldkv = coin(6) ? dim(3072, 1ll << 32) : d * uni(1, 3);
  tally(0, stlt_attn_grad_probs_cross(F<float>(1), ldq, F<float>(2), F<float>(3), ldkv, F<float>(4), F<uint8_t>(5), (int)uni(0, 1), S, Lq, Lk, H, dh, F<float>(6), s));
  // the shapes the fusion blocks have: always well-formed, so that the launch arithmetic itself runs
  const int64_t T = uni(1, 64), A = 33, Hh = uni(1, 12);
  tally(0, stlt_attn_grad_probs_cross(FA<float>(1), Hh * 64, FA<float>(2), FA<float>(3), 2 * Hh * 64, FA<float>(4), FA<uint8_t>(5), 0, uni(1, 4096), coin(2) ? T : A, coin(2) ? T : A, Hh,
                                      64, FA<float>(6), s));
  tally(0, stlt_attn_grad_probs_cross(FA<float>(1), 3 * Hh * 20, FA<float>(2), FA<float>(3), 3 * Hh * 20, FA<float>(4), FA<uint8_t>(5), 1, uni(1, 4096), T, T, Hh, 20, FA<float>(6), s));
  const int64_t n = coin(4) ? uni(-1, 66) : uni(0, 4), Tj = dim(64, 300), Aj = dim(33, 300), Sj = dim(2048, 1ll << 31);
  tally(1, stlt_attn_rollout_joint(coin(3) ? nullptr : F<float>(10), coin(3) ? nullptr : F<float>(11), F<float>(12), F<float>(13), F<float>(14), F<float>(15), n, Sj, Tj, Aj,
                                   F<float>(16), s));
  tally(1, stlt_attn_rollout_joint(FA<float>(10), FA<float>(11), FA<float>(12), FA<float>(13), FA<float>(14), FA<float>(15), uni(0, 64), uni(1, 1 << 20), uni(1, 256), uni(1, 256),
                                   FA<float>(16), s));
  const int64_t B = dim(1024, 1ll << 31), Tc = dim(64, 40000), Ac = dim(33, 40000), N = dim(36, 40000);
  tally(2, stlt_relevance_combine_joint(F<float>(20), F<float>(21), F<int64_t>(22), B, Tc, Ac, N, (float)uni(0, 1), (float)uni(0, 1), F<float>(23), F<float>(24), F<float>(25), s));
  tally(2, stlt_relevance_combine_joint(FA<float>(20), FA<float>(21), FA<int64_t>(22), uni(1, 4096), uni(1, 64), 33, uni(1, 36), 1.f, 1.f, FA<float>(23), FA<float>(24), FA<float>(25), s));
}

void fuzz_block() {
  void* s = nullptr;
  const int64_t d = coin(5) ? 4 * uni(0, 1024) : 64 * uni(1, 12), H = d > 0 && d % 64 == 0 ? d / 64 : dim(12, 64), S = dim(2048, 1ll << 24), Lq = dim(33, 300),
                Lk = coin(2) ? Lq : dim(33, 300);
  stlt_attn_block_params ap; { const float** f = reinterpret_cast<const float**>(&ap); for (int i = 0; i < 6; ++i) f[i] = FA<float>(30 + i); }
  const bool cross = coin(2);
  const int64_t rows = S > 0 && Lq > 0 && Lk > 0 && S < (1ll << 30) ? S * (Lq > Lk ? Lq : Lk) : 1;
  const size_t kb = coin(4) ? (size_t)uni(0, 1 << 20) : stlt_block_keep_bytes(rows, d, 0), wb = coin(4) ? (size_t)uni(0, 1 << 20) : stlt_block_work_bytes(rows, d);
  (void)stlt_gemm_set_scratch(coin(2) ? nullptr : FA<char>(29), coin(2) ? 0 : stlt_gemm_scratch_bytes());
  tally(3, stlt_attn_block_bwd_relevance(coin(40) ? nullptr : &ap, d, H, 1e-12f, F<float>(40), Lq, cross ? FA<float>(41) : nullptr, cross ? Lk : (coin(8) ? Lk : Lq), F<uint8_t>(42),
                                         (int)uni(0, 1), S, F<float>(43), cross ? F<float>(44) : nullptr, F<float>(45), F<float>(46), F<float>(47), F<float>(48),
                                         cross && coin(2) ? FA<float>(49) : nullptr, F<float>(50), F<char>(51), kb, F<char>(52), wb, s));
  (void)stlt_gemm_set_scratch(nullptr, 0);
}

stlt_layer_params fake_layer(int base) {
  stlt_layer_params l;
  const float** f = reinterpret_cast<const float**>(&l);
  for (size_t i = 0; i < sizeof(l) / sizeof(float*); ++i) f[i] = FA<float>(base + (int)i);
  return l;
}

void fuzz_backbone_sweep() {
  void* s = nullptr;
  stlt_params p{};
  p.d = coin(6) ? 4 * uni(0, 1024) : 64 * uni(1, 12);
  p.H = coin(6) ? dim(12, 64) : (p.d > 0 ? p.d / 64 : 0);
  p.n_categories = dim(38, 300);
  p.n_spatial = coin(8) ? uni(-1, 40) : uni(0, 4);
  p.n_temporal = coin(8) ? uni(-1, 40) : uni(0, 8);
  p.n_classes = dim(174, 5000);
  p.n_positions = coin(4) ? dim(256, 1024) : 256;
  p.ln_eps = 1e-12f;
  const float** f = &p.cat_emb;
  for (int i = 0; i < 11; ++i) f[i] = FA<float>(60 + i);
  if (coin(3)) p.score_w = p.score_b = nullptr;
  std::vector<stlt_layer_params> sp((size_t)(p.n_spatial > 0 ? p.n_spatial : 0), fake_layer(80)), tp((size_t)(p.n_temporal > 0 ? p.n_temporal : 0), fake_layer(100));
  p.spatial = sp.empty() ? nullptr : sp.data();
  p.temporal = tp.empty() ? nullptr : tp.data();
  stlt_inputs in{};
  in.B = dim(1024, 1ll << 22);
  in.T = dim(64, 300);
  in.N = dim(36, 300);
  in.categories = F<int64_t>(120); in.boxes = F<float>(121); in.scores = coin(2) || !p.score_w ? nullptr : FA<float>(122);
  in.kpm_boxes = F<uint8_t>(123); in.frame_types = F<int64_t>(124); in.kpm_frames = F<uint8_t>(125); in.lengths = F<int64_t>(126);
  const size_t tape = coin(4) ? (size_t)uni(0, 1 << 24) : stlt_train_tape_bytes(in.B, in.T, in.N, p.d, p.n_spatial, p.n_temporal);
  const size_t scr = coin(4) ? (size_t)uni(0, 1 << 24) : stlt_train_scratch_bytes(in.B, in.T, in.N, p.d, p.n_categories);
  const int flags = coin(4) ? (int)uni(0, 63) : 32;  // 32: STLT_FLAG_TRAIN_BACKBONE
  (void)stlt_train_forward(&p, &in, FA<char>(127), tape, FA<float>(128), 0.f, 0, flags, s);
  stlt_relevance_maps maps{};
  maps.abar_spatial = F<float>(130); maps.abar_temporal = F<float>(131); maps.rollout_spatial = F<float>(132); maps.rollout_temporal = F<float>(133);
  maps.relevance = (flags & 32) && !coin(6) ? nullptr : F<float>(134);  // must be NULL with the backbone flag, must not be without it
  tally(4, stlt_train_backward_relevance(coin(40) ? nullptr : &p, coin(40) ? nullptr : &in, F<char>(127), tape, FA<char>(135), scr, F<float>(136), coin(8) ? 0.1f : 0.f, rnd(), flags,
                                         nullptr, coin(40) ? nullptr : &maps, s));
}

}  // namespace

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 2000;
  g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
  if (stlt_version() != STLT_VERSION) { fprintf(stderr, "version mismatch\n"); return 2; }
  for (long i = 0; i < iters; ++i) {
    fuzz_ops();
    fuzz_block();
    fuzz_backbone_sweep();
  }
  printf("host_fuzz_fusion_relevance: calls that returned 0: grad_probs_cross %ld rollout_joint %ld combine_joint %ld block_bwd_relevance %ld backbone_sweep %ld\n", g_ok_by[0],
         g_ok_by[1], g_ok_by[2], g_ok_by[3], g_ok_by[4]);
  printf("host_fuzz_fusion_relevance: %ld iterations, %ld calls, %ld returned 0 (the rest refused their arguments); kernel launches configured: %ld , refused by the runtime: %ld ; last error: %s\n",
         iters, g_calls, g_ok, stlt_fake_hip_launches(), stlt_fake_hip_refused(), stlt_last_error());
  return 0;
}
