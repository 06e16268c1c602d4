// CAF / CACNF forward on precomputed appearance features (reference src/modelling/models.py:230-271, 286-298, 328-549).
// Pure orchestration of the kernels the STLT path already has (MFMA linear, attention core in its cross-attention
// form, residual+LayerNorm, gather) plus three tiny data-movement kernels.
#include "common.h"

namespace {

// (B, C, S) feature map -> token-major (B*S, C)
__global__ __launch_bounds__(256) void feat_transpose_kernel(const float* __restrict__ f, int C, int S, float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int64_t b = blockIdx.z;
  const int c0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, s = s0 + tx;
    tile[r][tx] = (c < C && s < S) ? f[(b * C + c) * (int64_t)S + s] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int s = s0 + r, c = c0 + tx;
    if (s < S && c < C) out[(b * S + s) * (int64_t)C + c] = tile[tx][r];
  }
}

// tokens (B, S+1, d): row 0 = cls + pos[0], row 1+s = proj[b,s] + pos[1+s]   (models.py:262-267)
__global__ __launch_bounds__(256) void app_assemble_kernel(const float* __restrict__ proj, const float* __restrict__ cls,
                                                           const float* __restrict__ pos, int S, int d, float* __restrict__ out) {
  const int64_t row = blockIdx.x;  // b*(S+1) + t
  const int t = (int)(row % (S + 1));
  const int64_t b = row / (S + 1);
  for (int e = threadIdx.x * 4; e < d; e += 1024) {
    f32x4 v = t == 0 ? *reinterpret_cast<const f32x4*>(cls + e) : *reinterpret_cast<const f32x4*>(proj + (b * S + (t - 1)) * (int64_t)d + e);
    v += *reinterpret_cast<const f32x4*>(pos + (int64_t)t * d + e);
    *reinterpret_cast<f32x4*>(out + row * d + e) = v;
  }
}

// out[b] = [a[b*lda : +d], c[b*ldc : +d]]  (torch.cat(..., dim=-1), models.py:470-476)
__global__ __launch_bounds__(256) void concat2_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ c, int64_t ldc,
                                                      int d, float* __restrict__ out) {
  const int64_t b = blockIdx.x;
  for (int e = threadIdx.x * 4; e < 2 * d; e += 1024) {
    const f32x4 v = e < d ? *reinterpret_cast<const f32x4*>(a + b * lda + e) : *reinterpret_cast<const f32x4*>(c + b * ldc + (e - d));
    *reinterpret_cast<f32x4*>(out + b * 2 * (int64_t)d + e) = v;
  }
}

__global__ __launch_bounds__(256) void mean3_kernel(const float* a, const float* b, const float* c, float* o, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) o[i] = ((a[i] + b[i]) + c[i]) / 3.0f;  // sum(logits) / 3, models.py:546
}

// the all-zero key-padding mask of the unmasked blocks, n bytes, as a kernel and not a memset: a memset node of a captured graph was seen to
// run out of order with the kernels around it on replay (ragged.hip: ragged_count_kernel), and the second replay of a captured fusion
// forward gave different appearance-branch results with the memset here (profiles/fusion_attention_bench.md, section 4)
__global__ __launch_bounds__(256) void zero_mask_kernel(uint8_t* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = 0;
}

struct CafWs {
  size_t bb, lh, ah, la, aa, q, kv, ctx, tmp, hh, ft, proj, zero, fused, h1, h2, hl, sk, total;
};

CafWs caf_ws(int64_t B, int64_t T, int64_t N, int64_t d, int64_t C, int64_t S, int64_t K) {
  CafWs w;
  const size_t f = sizeof(float);
  const size_t rows = (size_t)B * (T > S + 1 ? T : S + 1);
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = stlt_align256(off + bytes); return o; };
  w.bb = take(stlt_ws_bytes(B, T, N, d, K, 1));
  w.lh = take((size_t)B * T * d * f);
  w.ah = take((size_t)B * (S + 1) * d * f);
  w.la = take(rows * d * f);
  w.aa = take(rows * d * f);
  w.q = take(rows * 3 * d * f);   // also holds a packed qkv for the self-attention layers
  w.kv = take(rows * 2 * d * f);
  w.ctx = take(rows * d * f);
  w.tmp = take(rows * d * f);
  w.hh = take(rows * 4 * d * f);
  w.ft = take((size_t)B * S * C * f);
  w.proj = take((size_t)B * S * d * f);
  w.zero = take(rows);            // all-zero key-padding mask
  w.fused = take((size_t)B * 2 * d * f);
  w.h1 = take((size_t)B * d * f);
  w.h2 = take((size_t)B * d * f);
  w.hl = take((size_t)B * d * f);
  w.sk = take(STLT_GEMM_SCRATCH_BYTES);
  w.total = off;
  return w;
}

struct Bufs { float *q, *kv, *ctx, *tmp, *hh; const uint8_t* zero; };

// Where a block's attention probabilities go (stlt_caf_forward_attention): null = not asked for, no launch
struct Sink {
  float* probs = nullptr;
  int per_head = 0;
};

// Map `index` of a sink whose maps hold `rows` x `keys` probabilities per sequence (and per head with per_head)
Sink sink_at(float* base, int per_head, int64_t index, int64_t S, int64_t H, int64_t rows, int64_t keys) {
  return Sink{base ? base + (size_t)index * S * (per_head ? H : 1) * rows * keys : nullptr, per_head};
}

// SelfAttentionLayer (models.py:345-360): out = LN(MHA(x,x,x) + x)
int self_attn_block(const stlt_attn_block_params& p, int64_t d, int64_t H, float eps, const float* x, int64_t S, int64_t L,
                    const uint8_t* kpm, int causal, const Bufs& b, float* out, hipStream_t s, const Sink& sink = {}) {
  const int64_t M = S * L;
  TRY(launch_linear(x, d, p.in_proj_w, p.in_proj_b, b.q, 3 * d, M, 3 * d, d, STLT_ACT_NONE, s));
  TRY(launch_attn(b.q, kpm ? kpm : b.zero, causal, S, L, H, d / H, b.ctx, causal ? STLT_K_ATTN_TEMPORAL : STLT_K_ATTN_SPATIAL, s));
  if (sink.probs) TRY(launch_attn_probs(b.q, kpm ? kpm : b.zero, causal, S, L, H, d / H, sink.per_head, sink.probs, s));
  return stlt_linear_add_norm(b.ctx, d, d, p.out_proj_w, p.out_proj_b, x, d, p.ln_w, p.ln_b, eps, M, d, false, b.tmp, out, s);
}

// CrossAttentionLayer (models.py:362-382): out = LN(MHA(x, ctx, ctx, key_padding_mask) + x)
int cross_attn_block(const stlt_attn_block_params& p, int64_t d, int64_t H, float eps, const float* x, int64_t Lq, const float* c,
                     int64_t Lk, const uint8_t* kpm_k, int64_t S, const Bufs& b, float* out, hipStream_t s, const Sink& sink = {}) {
  TRY(launch_linear(x, d, p.in_proj_w, p.in_proj_b, b.q, d, S * Lq, d, d, STLT_ACT_NONE, s));                      // q rows of in_proj
  TRY(launch_linear(c, d, p.in_proj_w + d * d, p.in_proj_b + d, b.kv, 2 * d, S * Lk, 2 * d, d, STLT_ACT_NONE, s));  // k,v rows
  TRY(launch_attn_general(b.q, d, b.kv, b.kv + d, 2 * d, kpm_k ? kpm_k : b.zero, 0, S, Lq, Lk, H, d / H, b.ctx, STLT_K_ATTN_SPATIAL, s));
  if (sink.probs) TRY(launch_attn_probs_cross(b.q, d, b.kv, 2 * d, kpm_k ? kpm_k : b.zero, 0, S, Lq, Lk, H, d / H, sink.per_head, sink.probs, s));
  return stlt_linear_add_norm(b.ctx, d, d, p.out_proj_w, p.out_proj_b, x, d, p.ln_w, p.ln_b, eps, S * Lq, d, false, b.tmp, out, s);
}

// The fusion forward, written once.  attention == false: stlt_caf_forward_flags — the layout branch with the CLS-only elision and the fused
// kernels, `flags` may hold STLT_FLAG_SKIP_PADDING, no sinks.  attention == true: stlt_caf_forward_attention — the layout branch on the dense
// unfused schedule, and behind every attention core whose sink in `mp` is not null one probabilities launch on the core's own buffers and
// mask.  `who` opens the error messages.
int caf_forward_body(const char* who, bool attention, const stlt_caf_params* p, const stlt_inputs* in, const float* feats, void* workspace,
                     size_t workspace_bytes, int flags, int per_head, const stlt_caf_attention_maps& mp, float* logits_caf, float* logits_stlt,
                     float* logits_resnet3d, float* logits_ensemble, hipStream_t s) {
  if (!p || !in || !feats || !workspace || !logits_caf) return stlt_set_error(STLT_EINVAL, "%s: null argument", who);
  const stlt_params& lp = p->layout;
  const int64_t B = in->B, T = in->T, N = in->N, d = lp.d, H = lp.H, C = p->feat_channels, S = p->app_tokens, K = lp.n_classes;
  const float eps = lp.ln_eps;
  if (K <= 0 || !in->lengths || !p->fusion_head.fc1_w) return stlt_set_error(STLT_EINVAL, "%s: heads / lengths missing", who);
  if (B <= 0 || T <= 0 || N <= 0 || C <= 0 || S <= 0 || T > 256 || S > 4096 || N > 4096 || B > (int64_t)0x7fffffff / (T * N) || B > (int64_t)0x7fffffff / (S + 1) || K > 65536 ||
      C > 65536 || p->n_app_layers < 0 || p->n_fusion < 0 || (p->n_app_layers > 0 && !p->app_layers) || (p->n_fusion > 0 && !p->fusion))
    return stlt_set_error(STLT_EINVAL, "%s: bad shape (B %lld, T %lld, N %lld, feature channels %lld, appearance tokens %lld, classes %lld)", who, (long long)B,
                          (long long)T, (long long)N, (long long)C, (long long)S, (long long)K);
  if (C % 4 != 0 || !stlt_heads_ok(d, H)) return stlt_set_error(STLT_EINVAL, "%s: feat_channels and hidden_size must be multiples of 4, hidden_size %% heads == 0, head dim <= 256", who);
  const bool cacnf = p->layout_head.fc1_w != nullptr;
  if (cacnf && (!p->appearance_head.fc1_w || !logits_stlt || !logits_resnet3d || !logits_ensemble))
    return stlt_set_error(STLT_EINVAL, "%s: CACNF needs both unimodal heads and all four outputs", who);
  const CafWs w = caf_ws(B, T, N, d, C, S, K);
  if (attention) {  // everything that can refuse the call is looked at before the first launch
    if (workspace_bytes < w.total) return stlt_set_error(STLT_EINVAL, "%s: workspace %zu B < required %zu B", who, workspace_bytes, w.total);
    // T <= 256 is checked above: of a map's key counts only the object slots and the appearance tokens can exceed the kernels' 1024
    const bool fusion_maps = p->n_fusion > 0 && (mp.layout_to_appearance || mp.appearance_to_layout || mp.fusion_layout || mp.fusion_appearance);
    if ((mp.spatial && lp.n_spatial > 0 && N > 1024) || (((mp.appearance && p->n_app_layers > 0) || fusion_maps) && S + 1 > 1024))
      return stlt_set_error(STLT_EINVAL, "%s: a map over more than 1024 tokens (N=%lld, appearance tokens + 1 = %lld)", who, (long long)N, (long long)(S + 1));
    if (((uintptr_t)logits_caf | (uintptr_t)logits_stlt | (uintptr_t)logits_resnet3d | (uintptr_t)logits_ensemble | (uintptr_t)mp.spatial |
         (uintptr_t)mp.temporal | (uintptr_t)mp.appearance | (uintptr_t)mp.layout_to_appearance | (uintptr_t)mp.appearance_to_layout |
         (uintptr_t)mp.fusion_layout | (uintptr_t)mp.fusion_appearance) & 3)
      return stlt_set_error(STLT_EINVAL, "%s: the logits and the maps must be 4-byte aligned", who);
    if (!in->categories || !in->boxes || !in->kpm_boxes || !in->frame_types || !in->kpm_frames || T > lp.n_positions || lp.n_spatial < 0 || lp.n_temporal < 0 ||
        (lp.n_spatial && !lp.spatial) || (lp.n_temporal && !lp.temporal))
      return stlt_set_error(STLT_EINVAL, "%s: layout inputs / layer tables missing, or T=%lld beyond the position table", who, (long long)T);
  }
  if (workspace_bytes < w.total) return stlt_set_error(STLT_EWORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, w.total);
  if ((uintptr_t)workspace & 255) return stlt_set_error(STLT_EINVAL, "workspace must be 256-byte aligned");
  char* base = (char*)workspace;
  StltGemmScratch gemm_scratch(base + w.sk, STLT_GEMM_SCRATCH_BYTES);
  auto F = [&](size_t o) { return (float*)(base + o); };
  float *Lh = F(w.lh), *Ah = F(w.ah), *la = F(w.la), *aa = F(w.aa);
  Bufs b{F(w.q), F(w.kv), F(w.ctx), F(w.tmp), F(w.hh), (const uint8_t*)(base + w.zero)};
  const int64_t zero_bytes = B * (T > S + 1 ? T : S + 1);
  hipLaunchKernelGGL(zero_mask_kernel, dim3((unsigned)((zero_bytes + 255) / 256)), dim3(256), 0, s, (uint8_t*)(base + w.zero), zero_bytes);
  TRY(stlt_check_launch("zero_mask_kernel"));

  // ---- layout branch: full (B,T,d) backbone output (models.py:451); STLT_FLAG_SKIP_PADDING computes it on the real
  // tokens / frames only and leaves the padded frames' rows zero (they are masked keys everywhere downstream)
  if (attention)  // every row of every layer, each layer as the unfused pair: the towers of stlt_forward_attention (the elision flags do not apply)
    TRY(backbone_attention_public(&lp, in, base + w.bb, stlt_ws_bytes(B, T, N, d, K, 1), per_head, mp.spatial, mp.temporal, Lh, s));
  else
    TRY(backbone_impl_public(&lp, in, base + w.bb, stlt_ws_bytes(B, T, N, d, K, 1),
                             STLT_FLAG_CLS_ONLY_LAST_SPATIAL | (flags & STLT_FLAG_SKIP_PADDING), Lh, s));
  // ---- appearance branch from the feature map (models.py:253-271)
  hipLaunchKernelGGL(feat_transpose_kernel, dim3((unsigned)((C + 31) / 32), (unsigned)((S + 31) / 32), (unsigned)B), dim3(256), 0, s, feats,
                     (int)C, (int)S, F(w.ft));
  TRY(stlt_check_launch("feat_transpose_kernel"));
  TRY(launch_linear(F(w.ft), C, p->proj_w, p->proj_b, F(w.proj), d, B * S, d, C, STLT_ACT_NONE, s));
  hipLaunchKernelGGL(app_assemble_kernel, dim3((unsigned)(B * (S + 1))), dim3(256), 0, s, F(w.proj), p->cls_token, p->pos_embed, (int)S,
                     (int)d, Ah);
  TRY(stlt_check_launch("app_assemble_kernel"));
  const int64_t LA = S + 1, MA = B * LA, ML = B * T;
  for (int64_t l = 0; l < p->n_app_layers; ++l) {  // ReLU post-norm encoder layers, eps 1e-5, no masks
    const stlt_layer_params& e = p->app_layers[l];
    TRY(launch_linear(Ah, d, e.in_proj_w, e.in_proj_b, b.q, 3 * d, MA, 3 * d, d, STLT_ACT_NONE, s));
    TRY(launch_attn(b.q, b.zero, 0, B, LA, H, d / H, b.ctx, STLT_K_ATTN_SPATIAL, s));
    if (const Sink sk = sink_at(mp.appearance, per_head, l, B, H, LA, LA); sk.probs)
      TRY(launch_attn_probs(b.q, b.zero, 0, B, LA, H, d / H, sk.per_head, sk.probs, s));
    TRY(stlt_linear_add_norm(b.ctx, d, d, e.out_proj_w, e.out_proj_b, Ah, d, e.norm1_w, e.norm1_b, 1e-5f, MA, d, false, b.tmp, aa, s));
    TRY(stlt_ffn_norm(aa, d, e.lin1_w, e.lin1_b, STLT_ACT_RELU, e.lin2_w, e.lin2_b, e.norm2_w, e.norm2_b, 1e-5f, MA, d, false, b.hh, b.tmp, Ah, s));
  }
  // ---- unimodal states before fusion (models.py:459-460) -> CACNF heads
  if (cacnf) {
    TRY(launch_gather_last(Lh, in->lengths, B, T, d, F(w.hl), s));
    TRY(stlt_head(p->layout_head, F(w.hl), d, d, B, d, K, eps, F(w.h1), F(w.h2), logits_stlt, s));
    TRY(stlt_head(p->appearance_head, Ah, LA * d, d, B, d, K, eps, F(w.h1), F(w.h2), logits_resnet3d, s));  // rows (b, token 0)
  }
  // ---- multimodal fusion (models.py:462-468, 403-431)
  for (int64_t l = 0; l < p->n_fusion; ++l) {
    const stlt_crossmodal_params& m = p->fusion[l];
    TRY(cross_attn_block(m.cross_attn, d, H, eps, Lh, T, Ah, LA, nullptr, B, b, la, s,               // layout <- appearance
                         sink_at(mp.layout_to_appearance, per_head, l, B, H, T, LA)));
    TRY(cross_attn_block(m.cross_attn, d, H, eps, Ah, LA, Lh, T, in->kpm_frames, B, b, aa, s,        // appearance <- layout
                         sink_at(mp.appearance_to_layout, per_head, l, B, H, LA, T)));
    TRY(self_attn_block(m.layout_attn, d, H, eps, la, B, T, in->kpm_frames, 1, b, Lh, s,             // Lh = layout self-attn
                        sink_at(mp.fusion_layout, per_head, l, B, H, T, T)));
    TRY(self_attn_block(m.appearance_attn, d, H, eps, aa, B, LA, nullptr, 0, b, Ah, s,               // Ah = appearance self-attn
                        sink_at(mp.fusion_appearance, per_head, 2 * l, B, H, LA, LA)));
    // layout_ffn: LN(lin2(gelu(lin1(x))) + x)
    const stlt_ffn_block_params& f = m.layout_ffn;
    TRY(stlt_ffn_norm(Lh, d, f.lin1_w, f.lin1_b, STLT_ACT_GELU, f.lin2_w, f.lin2_b, f.ln_w, f.ln_b, eps, ML, d, false, b.hh, b.tmp, la, s));
    // appearance_ffn is a SelfAttentionLayer in the reference (models.py:401)
    TRY(self_attn_block(m.appearance_ffn, d, H, eps, Ah, B, LA, nullptr, 0, b, aa, s, sink_at(mp.fusion_appearance, per_head, 2 * l + 1, B, H, LA, LA)));
    float* t1 = Lh; Lh = la; la = t1;   // outputs of this module feed the next one
    float* t2 = Ah; Ah = aa; aa = t2;
  }
  // ---- fused state + FusionHead (models.py:470-476, 286-298)
  TRY(launch_gather_last(Lh, in->lengths, B, T, d, F(w.hl), s));
  hipLaunchKernelGGL(concat2_kernel, dim3((unsigned)B), dim3(256), 0, s, F(w.hl), d, Ah, LA * d, (int)d, F(w.fused));
  TRY(stlt_check_launch("concat2_kernel"));
  TRY(stlt_head(p->fusion_head, F(w.fused), 2 * d, 2 * d, B, d, K, eps, F(w.h1), F(w.h2), logits_caf, s));
  if (cacnf) {
    hipLaunchKernelGGL(mean3_kernel, dim3((unsigned)((B * K + 255) / 256)), dim3(256), 0, s, logits_stlt, logits_resnet3d, logits_caf,
                       logits_ensemble, B * K);
    TRY(stlt_check_launch("mean3_kernel"));
  }
  return 0;
}

}  // namespace

extern "C" size_t stlt_caf_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t feat_channels, int64_t app_tokens,
                                           int64_t n_classes) {
  if (B <= 0 || T <= 0 || N <= 0 || d <= 0 || feat_channels <= 0 || app_tokens <= 0) return 0;
  return caf_ws(B, T, N, d, feat_channels, app_tokens, n_classes).total;
}

extern "C" int stlt_caf_forward(const stlt_caf_params* p, const stlt_inputs* in, const float* feats, void* workspace,
                                size_t workspace_bytes, float* logits_caf, float* logits_stlt, float* logits_resnet3d,
                                float* logits_ensemble, stlt_stream_t stream) {
  return stlt_caf_forward_flags(p, in, feats, workspace, workspace_bytes, 0, logits_caf, logits_stlt, logits_resnet3d, logits_ensemble, stream);
}

extern "C" int stlt_caf_forward_flags(const stlt_caf_params* p, const stlt_inputs* in, const float* feats, void* workspace,
                                      size_t workspace_bytes, int flags, float* logits_caf, float* logits_stlt,
                                      float* logits_resnet3d, float* logits_ensemble, stlt_stream_t stream) {
  return caf_forward_body("stlt_caf_forward", false, p, in, feats, workspace, workspace_bytes, flags, 0, stlt_caf_attention_maps{}, logits_caf, logits_stlt,
                          logits_resnet3d, logits_ensemble, (hipStream_t)stream);
}

extern "C" size_t stlt_caf_attention_workspace_bytes(int64_t B, int64_t T, int64_t N, int64_t d, int64_t feat_channels, int64_t app_tokens,
                                                     int64_t n_classes) {
  return stlt_caf_workspace_bytes(B, T, N, d, feat_channels, app_tokens, n_classes);  // the same buffers: every block's Q / K already lie in them
}

extern "C" int stlt_caf_forward_attention(const stlt_caf_params* p, const stlt_inputs* in, const float* feats, void* workspace,
                                          size_t workspace_bytes, int flags, int per_head, float* logits_caf, float* logits_stlt,
                                          float* logits_resnet3d, float* logits_ensemble, const stlt_caf_attention_maps* maps,
                                          stlt_stream_t stream) {
  if (flags & STLT_FLAG_SKIP_PADDING)
    return stlt_set_error(STLT_EINVAL, "stlt_caf_forward_attention: STLT_FLAG_SKIP_PADDING is not supported (the attention maps are those of the padded schedule)");
  if (per_head != 0 && per_head != 1) return stlt_set_error(STLT_EINVAL, "stlt_caf_forward_attention: per_head must be 0 or 1");
  return caf_forward_body("stlt_caf_forward_attention", true, p, in, feats, workspace, workspace_bytes, 0, per_head, maps ? *maps : stlt_caf_attention_maps{},
                          logits_caf, logits_stlt, logits_resnet3d, logits_ensemble, (hipStream_t)stream);
}
