// Per-pixel arithmetic shared by the device video collater (video.hip) and the device frame store (frame_store.hip): Pillow's 8-bit
// rounding of a resample accumulator, convert("L"), Image.blend, F_pil.adjust_hue and VideoColorJitter's op chain
// (src/utils/data_utils.py:110-137), restated so that both paths give the reference's values bit for bit.  Blends are Image.blend's
// float32 arithmetic; HSV follows libImaging/Convert.c (float32 variables, float64 literals).  Include it after
// `#pragma clang fp contract(off)`: no contraction anywhere below.
#pragma once
#include "common.h"

#include <math.h>

namespace {

constexpr int VP_PREC = 22;  // Pillow's PRECISION_BITS for 8-bit images

__device__ inline int vp_clip8(int acc) {
  if (acc >= (1 << VP_PREC << 8)) return 255;
  if (acc <= 0) return 0;
  return acc >> VP_PREC;
}

struct Px {
  int c[3];
};

__device__ inline int vp_luma(const Px& p) { return (p.c[0] * 19595 + p.c[1] * 38470 + p.c[2] * 7471 + 0x8000) >> 16; }

// Image.blend(in1, in2, alpha): float32 in1 + alpha * (in2 - in1), clipped, truncated
__device__ inline int vp_blend(int in1, int in2, float alpha) {
  const float t = (float)in1 + alpha * (float)(in2 - in1);
  if (t <= 0.f) return 0;
  if (t >= 255.f) return 255;
  return (int)t;
}

// F_pil.adjust_hue: RGB -> HSV (rgb2hsv_row), uint8 add to H, HSV -> RGB (hsv2rgb)
__device__ inline Px vp_hue(const Px& in, int shift) {
  const int r = in.c[0], g = in.c[1], b = in.c[2];
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = maxc;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double q = (double)h / 6.0 + 1.0;  // in [5/6, 11/6]: fmod(q, 1.0) is q - 1 above 1, exactly
    h = (float)(q >= 1.0 ? q - 1.0 : q);
    uh = min(max((int)((double)h * 255.0), 0), 255);
    us = min(max((int)((double)s * 255.0), 0), 255);
  }
  uh = (uh + shift) & 255;
  Px o;
  if (us == 0) {
    o.c[0] = o.c[1] = o.c[2] = uv;
    return o;
  }
  const double h6 = (double)(float)uh * 6.0 / 255.0;
  const int i = (int)floor(h6);
  const float f = (float)(h6 - (double)(float)i);
  const float fs = (float)((double)(float)us / 255.0);
  const double v = (double)(float)uv;
  const int p = min(max((int)round(v * (1.0 - (double)fs)), 0), 255);
  const int q = min(max((int)round(v * (1.0 - (double)(fs * f))), 0), 255);
  const int t = min(max((int)round(v * (1.0 - (double)fs * (1.0 - (double)f))), 0), 255);
  switch (i % 6) {
    case 0: o.c[0] = uv; o.c[1] = t; o.c[2] = p; break;
    case 1: o.c[0] = q; o.c[1] = uv; o.c[2] = p; break;
    case 2: o.c[0] = p; o.c[1] = uv; o.c[2] = t; break;
    case 3: o.c[0] = p; o.c[1] = q; o.c[2] = uv; break;
    case 4: o.c[0] = t; o.c[1] = p; o.c[2] = uv; break;
    default: o.c[0] = uv; o.c[1] = p; o.c[2] = q; break;
  }
  return o;
}

// ops order[from, to) of VideoColorJitter on one pixel (Clip: stlt_video_clip or stlt_frames_clip); mean = the frame's contrast level (unused before contrast)
template <typename Clip>
__device__ inline Px vp_jitter(Px p, const Clip& d, int from, int to, int mean) {
  for (int o = from; o < to; ++o) {
    const int fn = d.order[o];
    if (fn == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.c[c] = vp_blend(0, p.c[c], d.brightness);
    } else if (fn == 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.c[c] = vp_blend(mean, p.c[c], d.contrast);
    } else if (fn == 2) {
      const int l = vp_luma(p);
#pragma unroll
      for (int c = 0; c < 3; ++c) p.c[c] = vp_blend(l, p.c[c], d.saturation);
    } else {
      p = vp_hue(p, d.hue_shift);
    }
  }
  return p;
}

template <typename Clip>
__device__ inline int vp_contrast_pos(const Clip& d) {
  int pos = 0;
  for (int o = 0; o < 4; ++o)
    if (d.order[o] == 1) pos = o;
  return pos;
}

}  // namespace
