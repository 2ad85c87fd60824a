// Streaming pose tracker core: this frame's crop from the last frame's key-point estimate.  Plain inline functions, the same for
// the kernels of track.hip and for a host compiler (tests/track_host_check.cpp): TRK_HD is the only thing that differs.
//
// Replaces, fed the PREDICTED key-points, what the reference's loader computes from the annotated ones:
//   lib/dataset/dream.py:171-216, 287-394     bbox_gt2d, the crop box, both views' K / boxes
//   lib/dataset/roboutils.py:59-156, 224-257  get_bbox, resize_image, bbox_transform, get_extended_bbox
//   lib/utils/geometries.py:360-395           get_K_crop_resize
//   lib/core/function.py:43-48, 88-98         the box / K selection and k_values
//
// Arithmetic rules: float64 where the loader computes in float64 numpy, float32 where it computes in float32 torch, in its order of
// operations, int() truncation where it truncates, and NO contraction: the pragma below switches it off for clang / hipcc, the
// host check program is also built with -ffp-contract=off; the three fused steps of the bilinear resize that torch's CPU kernel
// contracts are explicit fmaf calls (dream.hip:206-215).
// Safety rules, held by tests/track_host_check.cpp under ASan / UBSan: a value is range-checked before every float -> int
// conversion (NaN or 1e300 never reaches a cast); every frame index is tested against W, H immediately before its load, whatever
// the record says.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/hrp.h"

#if defined(__HIPCC__)
#define TRK_HD __host__ __device__ inline
#else
#define TRK_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace track {

// correctly rounded fp32 division and square root, whatever the device compile flags say
TRK_HD float fdiv(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}
TRK_HD float fsqrt(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsqrt_rn(a);
#else
  return sqrtf(a);
#endif
}

TRK_HD bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN and +-inf
TRK_HD bool finite32(float v) { return fabsf(v) <= 3.402823466e38f; }
// Python's max(0, v) and min(w, v): the first argument unless the comparison holds (so NaN gives the bound)
TRK_HD double max0(double v) { return v > 0.0 ? v : 0.0; }
TRK_HD double minw(double w, double v) { return v < w ? v : w; }
TRK_HD int imin(int a, int b) { return a < b ? a : b; }
TRK_HD int imax(int a, int b) { return a > b ? a : b; }
// int(v) of a value the loader truncates; false when it would not fit (the loader's box then fails its own check as well)
TRK_HD bool to_int(double v, int& out) {
  if (!(v >= -1073741824.0 && v <= 1073741824.0)) return false;
  out = (int)v;
  return true;
}

// The points a box is made from: the nkp key-points of the estimate, or (n == 0) the four corners of the whole frame
struct Points {
  const double* kp;
  int n, W, H;
};
TRK_HD int count(const Points& p) { return p.n ? p.n : 4; }
TRK_HD double px(const Points& p, int i) { return p.n ? p.kp[2 * i] : ((i == 1 || i == 2) ? (double)p.W : 0.0); }
TRK_HD double py(const Points& p, int i) { return p.n ? p.kp[2 * i + 1] : (i >= 2 ? (double)p.H : 0.0); }

struct Views {
  int h[2], w[2];      // h = min, w = max of resize_hw; boxes: x bounded by resize_hw[0] = h, y by resize_hw[1] = w, as the reference
  int two;             // 0: the views have one size, view 1 is a copy of view 0
};

// One view (_get_rootnet_data / _get_other_data, dream.py:287-394, without the pixels): K, bbox_strict_bounded, bbox_gt2d_extended
TRK_HD void view_geometry(const Points& p, const float* Ko, const double* Kc, const hrp_track_geom& g, int h, int w, double er0,
                          double er1, float* Kv, float* strict, float* ext) {
  const bool resized = !(g.side == h && g.side == w);
  double k00, k02, k11, k12;                 // the view's K as float64, what bbox_transform and the key-point mapping multiply by
  for (int i = 0; i < 9; ++i) Kv[i] = (float)Kc[i];
  if (resized) {                             // get_K_crop_resize in float32 on the box [0, 0, side, side] (geometries.py:360-395)
    const float fw = (float)w, fh = (float)h, cw = (float)g.side, ch = (float)g.side;
    const float cj = fdiv(0.f + cw, 2.f), ci = fdiv(0.f + ch, 2.f);
    const float hx = fdiv(cw - 1.f, 2.f), hy = fdiv(ch - 1.f, 2.f);
    const float cx = (Kv[2] + hx) - cj, cy = (Kv[5] + hy) - ci;
    const float dx = cx - hx, dy = cy - hy;
    const float sx = fdiv(fw, cw), sy = fdiv(fh, ch);
    const float n00 = sx * Kv[0], n11 = sy * Kv[4];
    const float n02 = fdiv(fw - 1.f, 2.f) + sx * dx, n12 = fdiv(fh - 1.f, 2.f) + sy * dy;
    Kv[0] = n00;
    Kv[4] = n11;
    Kv[2] = n02;
    Kv[5] = n12;
    k00 = (double)n00, k02 = (double)n02, k11 = (double)n11, k12 = (double)n12;
  } else {                                   // side == out: the canvas K unchanged (augmentations.py:176-178)
    k00 = Kc[0], k02 = Kc[2], k11 = Kc[4], k12 = Kc[5];
  }
  const double fx = (double)Ko[0], cx0 = (double)Ko[2], fy = (double)Ko[4], cy0 = (double)Ko[5];
  const double xlim = (double)h, ylim = (double)w;
  // bbox_transform (roboutils.py:224-242): corners through K_original^-1 (the ray) and the view's K, clipped
  const float* so = g.bbox_strict_bounded_original;
  strict[0] = (float)minw(xlim, max0(k00 * (((double)so[0] - cx0) / fx) + k02));
  strict[1] = (float)minw(ylim, max0(k11 * (((double)so[1] - cy0) / fy) + k12));
  strict[2] = (float)minw(xlim, max0(k00 * (((double)so[2] - cx0) / fx) + k02));
  strict[3] = (float)minw(ylim, max0(k11 * (((double)so[3] - cy0) / fy) + k12));
  // the key-points in the view: K_view @ kp3d / z with kp3d on the ray of the original pixel; the canvas shift when not resized
  double g0 = 0, g1 = 0, g2 = 0, g3 = 0;
  const int n = count(p);
  for (int i = 0; i < n; ++i) {
    const double u = px(p, i), v = py(p, i);
    double x, y;
    if (resized) {
      x = k00 * ((u - cx0) / fx) + k02;
      y = k11 * ((v - cy0) / fy) + k12;
    } else {
      x = (u + (double)g.off_x) - (double)g.crop_x0;
      y = (v - (double)g.crop_y0) + (double)g.off_y;
    }
    if (i == 0) {
      g0 = g2 = x;
      g1 = g3 = y;
    } else {
      g0 = x < g0 ? x : g0;
      g1 = y < g1 ? y : g1;
      g2 = x > g2 ? x : g2;
      g3 = y > g3 ? y : g3;
    }
  }
  const double bw = g2 - g0, bh = g3 - g1;   // get_extended_bbox (roboutils.py:244-257), bounded
  ext[0] = (float)max0(g0 - bw * er0);
  ext[1] = (float)max0(g1 - bh * er1);
  ext[2] = (float)minw(xlim, g2 + bw * er0);
  ext[3] = (float)minw(ylim, g3 + bh * er1);
}

// compute_k_values' float32 formula (function.py:88-98): sqrt(fx * fy * 1000 * 1000 / max(|x1 - x0|, |y1 - y0|)^2)
TRK_HD float k_value_of(float fx, float fy, const float* b) {
  const float a = fmaxf(fabsf(b[2] - b[0]), fabsf(b[3] - b[1]));
  return fsqrt(fdiv(((fx * fy) * 1000.f) * 1000.f, a * a));
}

// The whole path for one set of points.  false: the loader would have refused this box (or k_value / an input is unusable); the
// crop fields of g are written only when the box itself is good.
TRK_HD bool geometry_from(const Points& p, const float* Ko, int W, int H, const Views& vw, double er0, double er1, int bbox_mode,
                          hrp_track_geom& g, float* K_root, float* K_other, float& k_value) {
  const int n = count(p);
  double b0 = 0, b1 = 0, b2 = 0, b3 = 0;      // bbox_gt2d: min / max of the key-points (dream.py:257-258)
  for (int i = 0; i < n; ++i) {
    const double u = px(p, i), v = py(p, i);
    if (!finite64(u) || !finite64(v)) return false;
    if (i == 0) {
      b0 = b2 = u;
      b1 = b3 = v;
    } else {
      b0 = u < b0 ? u : b0;
      b1 = v < b1 ? v : b1;
      b2 = u > b2 ? u : b2;
      b3 = v > b3 ? v : b3;
    }
  }
  {                                           // get_bbox(strict=True) (roboutils.py:59-103)
    const double w = (double)W, h = (double)H;
    const double x0 = max0(b0), y0 = max0(b1), x1 = minw(w, b2), y1 = minw(h, b3);
    const double bw = x1 - x0, bh = y1 - y0;
    int ix0, iy0, ix1, iy1;
    if (!to_int(max0(x0 - 0.3 * bw), ix0) || !to_int(minw(w, x1 + 0.3 * bw), ix1)) return false;
    if (!to_int(max0(y0 - 0.3 * bh), iy0) || !to_int(minw(h, y1 + 0.3 * bh), iy1)) return false;
    if (ix1 - ix0 < 150) {
      ix1 += 75;
      ix0 -= 75;
    }
    if (iy1 - iy0 < 120) {
      iy1 += 60;
      iy0 -= 60;
    }
    ix0 = imax(0, ix0), iy0 = imax(0, iy0), ix1 = imin(W, ix1), iy1 = imin(H, iy1);
    ix0 = imin(W, ix0), iy0 = imin(H, iy0), ix1 = imax(0, ix1), iy1 = imax(0, iy1);
    if (!(0 <= ix0 && ix0 < ix1 && ix1 <= W && 0 <= iy0 && iy0 < iy1 && iy1 <= H)) return false;     // dream.py:318
    g.crop_x0 = ix0, g.crop_y0 = iy0, g.crop_x1 = ix1, g.crop_y1 = iy1;
    const int cw = ix1 - ix0, ch = iy1 - iy0;    // resize_image's canvas (roboutils.py:124-150)
    g.side = imax(cw, ch);
    g.off_x = (g.side - cw) / 2;
    g.off_y = (g.side - ch) / 2;
  }
  for (int i = 0; i < 9; ++i)
    if (!finite32(Ko[i])) return false;
  if (Ko[0] == 0.f || Ko[4] == 0.f || !finite64(er0) || !finite64(er1)) return false;
  double Kc[9];                               // the canvas K, float64 (_resize_geometry)
  for (int i = 0; i < 9; ++i) Kc[i] = (double)Ko[i];
  Kc[2] = Kc[2] - (double)(g.crop_x0 - g.off_x);
  Kc[5] = Kc[5] - (double)(g.crop_y0 - g.off_y);
  // with no annotated bounding_box: get_extended_bbox(bbox_gt2d, 20, 20, 20, 20, bounded, (W, H)) as a FloatTensor (dream.py:261-267)
  g.bbox_strict_bounded_original[0] = (float)max0(b0 - 20.0);
  g.bbox_strict_bounded_original[1] = (float)max0(b1 - 20.0);
  g.bbox_strict_bounded_original[2] = (float)minw((double)W, b2 + 20.0);
  g.bbox_strict_bounded_original[3] = (float)minw((double)H, b3 + 20.0);
  view_geometry(p, Ko, Kc, g, vw.h[0], vw.w[0], er0, er1, K_root, g.bbox_strict_bounded[0], g.bbox_gt2d_extended[0]);
  if (vw.two) {
    view_geometry(p, Ko, Kc, g, vw.h[1], vw.w[1], er0, er1, K_other, g.bbox_strict_bounded[1], g.bbox_gt2d_extended[1]);
  } else {
    for (int i = 0; i < 9; ++i) K_other[i] = K_root[i];
    for (int i = 0; i < 4; ++i) {
      g.bbox_strict_bounded[1][i] = g.bbox_strict_bounded[0][i];
      g.bbox_gt2d_extended[1][i] = g.bbox_gt2d_extended[0][i];
    }
  }
  // the box and K that k_values is computed from (function.py:43-48, 89-94): the root view's, or the original image's
  if (bbox_mode == HRP_TRACK_BBOX_ORIGIN)
    k_value = k_value_of(Ko[0], Ko[4], g.bbox_strict_bounded_original);
  else
    k_value = k_value_of(K_root[0], K_root[4],
                         bbox_mode == HRP_TRACK_BBOX_EXTENDED ? g.bbox_gt2d_extended[0] : g.bbox_strict_bounded[0]);
  return finite32(k_value) && k_value > 0.f;
}

// One stream's record for this frame.  kp2d [nkp][2] float64 in ORIGINAL-image pixels; have: 0 = no estimate.  An estimate the
// loader would refuse is treated as absent: the whole frame [0, 0, W, H] is taken, its corners stand in for the key-points, and
// HRP_TRACK_BAD_BOX | HRP_TRACK_NO_ESTIMATE is set.  Should even the whole frame give no usable k_value (K_original or
// extend_ratio not finite or degenerate), k_value is 1 and K_root / K_other are K_original: floats only, never an index.
TRK_HD void track_geometry(const double* kp2d, int nkp, int have, const float* K_original, int W, int H, const Views& vw, double er0,
                           double er1, int bbox_mode, hrp_track_geom& g, float* K_root, float* K_other, float& k_value) {
  int status = 0;
  bool ok = false;
  if (have) {
    const Points p = {kp2d, nkp, W, H};
    ok = geometry_from(p, K_original, W, H, vw, er0, er1, bbox_mode, g, K_root, K_other, k_value);
    if (!ok) status |= HRP_TRACK_BAD_BOX;
  }
  if (!ok) {
    status |= HRP_TRACK_NO_ESTIMATE;
    const Points p = {nullptr, 0, W, H};
    if (!geometry_from(p, K_original, W, H, vw, er0, er1, bbox_mode, g, K_root, K_other, k_value)) {
      status |= HRP_TRACK_BAD_BOX;
      k_value = 1.f;
      for (int i = 0; i < 9; ++i) K_root[i] = K_other[i] = K_original[i];
      for (int i = 0; i < 4; ++i) {
        g.bbox_strict_bounded[0][i] = g.bbox_strict_bounded[1][i] = 0.f;
        g.bbox_gt2d_extended[0][i] = g.bbox_gt2d_extended[1][i] = 0.f;
        g.bbox_strict_bounded_original[i] = 0.f;
      }
    }
  }
  g.status = status;
}

// ---- pixels -------------------------------------------------------------------------------------------------------------------
// canvas pixel (cx, cy) of resize_image's zero-padded side x side square, read from the frame itself
TRK_HD void canvas_px(const uint8_t* frame, int W, int H, const hrp_track_geom& g, int cx, int cy, int* v) {
  const int x = cx - g.off_x + g.crop_x0, y = cy - g.off_y + g.crop_y0;
  v[0] = v[1] = v[2] = 0;
  if (x < g.crop_x0 || x >= g.crop_x1 || y < g.crop_y0 || y >= g.crop_y1) return;
  if (x < 0 || y < 0 || x >= W || y >= H) return;            // the frame's own bounds, whatever the record says
  const uint8_t* q = frame + ((int64_t)y * W + x) * 3;
  v[0] = q[0];
  v[1] = q[1];
  v[2] = q[2];
}

// torch's CPU bilinear source index (align_corners=False): area_pixel_compute_source_index + guard_index_and_lambda
TRK_HD void src_index(int o, int in_size, float scale, int& i0, int& i1, float& l0, float& l1) {
  float r = scale * ((float)o + 0.5f) - 0.5f;
  r = r < 0.f ? 0.f : r;                                     // r <= 4096 * 4096: the cast below is in range
  i0 = imin((int)floorf(r), in_size - 1);
  l1 = r - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l0 = 1.f - l1;
}

TRK_HD float u8f(int v) { return fdiv((float)v, 255.f); }

// a record whose integers cannot overflow the index arithmetic below; any other gives a black view
TRK_HD bool record_ok(const hrp_track_geom& g) {
  const int M = HRP_TRACK_MAX_SIZE;
  return g.side >= 1 && g.side <= M && g.off_x >= 0 && g.off_x <= M && g.off_y >= 0 && g.off_y <= M && g.crop_x0 >= 0 &&
         g.crop_x0 <= M && g.crop_y0 >= 0 && g.crop_y0 <= M && g.crop_x1 >= 0 && g.crop_x1 <= M && g.crop_y1 >= 0 && g.crop_y1 <= M;
}

// Output pixel (ox, oy) of an h x w view: dream_crop_resize_kernel's arithmetic without the enhancement tail.  frame: one
// [H, W, 3] uint8 frame.
TRK_HD void track_pixel(const uint8_t* frame, int W, int H, const hrp_track_geom& g, int h, int w, int ox, int oy, uint8_t* rgb) {
  const int S = g.side;
  int r[3] = {0, 0, 0};
  if (record_ok(g)) {
    if (S == h && S == w) {
      canvas_px(frame, W, H, g, ox, oy, r);
    } else {
      const float sy = fdiv((float)S, (float)h), sx = fdiv((float)S, (float)w);
      int y0, y1, x0, x1;
      float ly0, ly1, lx0, lx1;
      src_index(oy, S, sy, y0, y1, ly0, ly1);
      src_index(ox, S, sx, x0, x1, lx0, lx1);
      int v00[3], v01[3], v10[3], v11[3];
      canvas_px(frame, W, H, g, x0, y0, v00);
      canvas_px(frame, W, H, g, x1, y0, v01);
      canvas_px(frame, W, H, g, x0, y1, v10);
      canvas_px(frame, W, H, g, x1, y1, v11);
      for (int c = 0; c < 3; ++c) {
        // torch's generic CPU kernel contracts t0 * w0 + t1 * w1 to fma(t0, w0, t1 * w1) (dream.hip:206-215)
        const float t0 = fmaf(u8f(v00[c]), lx0, u8f(v01[c]) * lx1);
        const float t1 = fmaf(u8f(v10[c]), lx0, u8f(v11[c]) * lx1);
        const float o = fmaf(t0, ly0, t1 * ly1);
        const float s = o * 255.f;
        r[c] = s <= 0.f ? 0 : (s >= 255.f ? 255 : (int)s);
      }
    }
  }
  rgb[0] = (uint8_t)r[0];
  rgb[1] = (uint8_t)r[1];
  rgb[2] = (uint8_t)r[2];
}

// ---- the estimate from the model's output -------------------------------------------------------------------------------------
// xyz [nkp][3] fp32, camera frame -> kp2d = (fx X / Z + cx, fy Y / Z + cy) in float64 (geometries.py:100-115 on K_original), written
// to state [nkp][2] and, as fp32, to out [nkp][2].  Returns have: every coordinate finite, every Z > 0, and at least min_inside
// key-points in [0, W) x [0, H).
TRK_HD int track_update(const float* xyz, int nkp, const float* K_original, int W, int H, int min_inside, double* state, float* out) {
  const double fx = (double)K_original[0], cx = (double)K_original[2], fy = (double)K_original[4], cy = (double)K_original[5];
  bool good = finite64(fx) && finite64(cx) && finite64(fy) && finite64(cy);
  int inside = 0;
  for (int i = 0; i < nkp; ++i) {
    const double X = (double)xyz[3 * i], Y = (double)xyz[3 * i + 1], Z = (double)xyz[3 * i + 2];
    const double u = fx * X / Z + cx, v = fy * Y / Z + cy;
    state[2 * i] = u;
    state[2 * i + 1] = v;
    out[2 * i] = (float)u;
    out[2 * i + 1] = (float)v;
    good = good && finite64(X) && finite64(Y) && finite64(Z) && Z > 0.0 && finite64(u) && finite64(v);
    if (u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H) ++inside;
  }
  return (good && inside >= min_inside) ? 1 : 0;
}

// ---- acquisition: the estimate from a detector's key-points -------------------------------------------------------------------
// det [nkp][2] fp32 in DETECTOR pixels (x, y), inv_sx / inv_sy frame pixels per detector pixel; mask [hm][wm] fp32 at detector
// resolution or null; ms [nkp][2] (max logit, sum exp) or null.  have != 0 without force: HRP_SEED_SKIPPED, nothing is written.
// Otherwise u = (double)det * inv_scale; a key-point counts when it is finite, lies in [0, W) x [0, H), the mask at its truncated
// detector pixel is >= min_prob and its peak probability 1 / sum-exp is >= min_peak.  Every key-point finite and at least
// min_inside counting: all nkp points are written to state [nkp][2], have = 1, HRP_SEED_TAKEN; else nothing is written,
// HRP_SEED_REFUSED.  The mask index is formed only from values already tested against [0, wm) x [0, hm).
TRK_HD int track_seed(const float* det, int nkp, double inv_sx, double inv_sy, const float* mask, int hm, int wm, float min_prob,
                      const float* ms, float min_peak, int min_inside, int force, int W, int H, double* state, int32_t& have) {
  if (have && !force) return HRP_SEED_SKIPPED;
  bool finite = finite64(inv_sx) && finite64(inv_sy);
  int counted = 0;
  for (int i = 0; i < nkp; ++i) {
    const float dx = det[2 * i], dy = det[2 * i + 1];
    const double u = (double)dx * inv_sx, v = (double)dy * inv_sy;
    if (!finite32(dx) || !finite32(dy) || !finite64(u) || !finite64(v)) {
      finite = false;
      continue;
    }
    bool ok = u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H;
    if (ok && mask) {
      ok = dx >= 0.f && dx < (float)wm && dy >= 0.f && dy < (float)hm;       // tested first: the casts below are in range
      if (ok) {
        const int mx = (int)dx, my = (int)dy;
        ok = mx >= 0 && mx < wm && my >= 0 && my < hm && mask[(int64_t)my * wm + mx] >= min_prob;
      }
    }
    if (ok && ms) ok = fdiv(1.f, ms[2 * i + 1]) >= min_peak;                 // (NaN compares false)
    if (ok) ++counted;
  }
  if (!finite || counted < min_inside) return HRP_SEED_REFUSED;
  for (int i = 0; i < nkp; ++i) {
    state[2 * i] = (double)det[2 * i] * inv_sx;
    state[2 * i + 1] = (double)det[2 * i + 1] * inv_sy;
  }
  have = 1;
  return HRP_SEED_TAKEN;
}

// ---- verification: the estimate against the detector's foreground map ----------------------------------------------------------
// The rule of include/hrp.h (hrp_track_verify) in the pieces the kernel shares out among its lanes: verify_geometry once per
// stream, verify_sample per sample point, verify_pixel per pixel, verify_decide once on the totals.  track_verify below is the
// same rule for one stream in one thread (tests/track_verify_host_check.cpp); only the order of the float64 sums differs.
struct VerifyGeom {
  double d[HRP_TRACK_MAX_KP][2];     // the key-points in detector pixels
  double box[4];                     // the extended box of step 4
};
struct VerifyAcc {
  double I, S, R;
  int n_fg, n_in;
};

// steps 0 - 2 and the box: 0 to go on, otherwise the stream's final status (HRP_VERIFY_SKIPPED, or HRP_VERIFY_DROPPED)
TRK_HD int verify_geometry(const double* kp2d, int nkp, int have, double sx, double sy, double er0, double er1, VerifyGeom& g) {
  if (!have) return HRP_VERIFY_SKIPPED;
  double x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  for (int i = 0; i < nkp; ++i) {
    const double u = kp2d[2 * i], v = kp2d[2 * i + 1];
    const double x = u * sx, y = v * sy;
    if (!finite64(u) || !finite64(v) || !finite64(x) || !finite64(y)) return HRP_VERIFY_DROPPED;
    g.d[i][0] = x;
    g.d[i][1] = y;
    if (i == 0) {
      x0 = x1 = x;
      y0 = y1 = y;
    } else {
      x0 = x < x0 ? x : x0;
      y0 = y < y0 ? y : y0;
      x1 = x > x1 ? x : x1;
      y1 = y > y1 ? y : y1;
    }
  }
  const double w = x1 - x0, h = y1 - y0;
  g.box[0] = x0 - er0 * w;
  g.box[1] = y0 - er1 * h;
  g.box[2] = x1 + er0 * w;
  g.box[3] = y1 + er1 * h;
  return 0;
}

TRK_HD int verify_samples(int nkp, int nb, int S) { return nkp + nb * S; }

// sample s of nkp + nb * S: the key-points first, then S points along every bone.  The mask index is formed only from values
// already tested against [0, wm) x [0, hm) in double, and tested again as integers before the load.
TRK_HD void verify_sample(const VerifyGeom& g, int nkp, const int32_t (*bones)[2], int S, int s, const float* mask, int hm, int wm,
                          float min_prob, int& counted, int& hit) {
  double x, y;
  if (s < nkp) {
    x = g.d[s][0];
    y = g.d[s][1];
  } else {
    const int k = (s - nkp) / S, j = (s - nkp) % S;
    const int a = bones[k][0], b = bones[k][1];
    if (a < 0 || a >= nkp || b < 0 || b >= nkp) return;      // (the entry point refuses such a bone)
    const double t = ((double)j + 0.5) / (double)S;
    x = g.d[a][0] + t * (g.d[b][0] - g.d[a][0]);
    y = g.d[a][1] + t * (g.d[b][1] - g.d[a][1]);
  }
  if (!(x >= 0.0 && x < (double)wm && y >= 0.0 && y < (double)hm)) return;
  const int ix = (int)x, iy = (int)y;
  if (ix < 0 || ix >= wm || iy < 0 || iy >= hm) return;
  ++counted;
  if (mask[(int64_t)iy * wm + ix] >= min_prob) ++hit;
}

// pixel (x, y) with mask value m and silhouette value a (read only when use_alpha)
TRK_HD void verify_pixel(const VerifyGeom& g, float m, float a, bool use_alpha, int x, int y, float min_prob, VerifyAcc& acc) {
  const double md = (double)m;
  acc.S += md;
  if (use_alpha) {
    const double ad = (double)a;
    acc.R += ad;
    acc.I += md * ad;
  }
  if (m >= min_prob) {
    ++acc.n_fg;
    const double cx = (double)x + 0.5, cy = (double)y + 0.5;
    if (cx >= g.box[0] && cx <= g.box[2] && cy >= g.box[1] && cy <= g.box[3]) ++acc.n_in;
  }
}

// step 6 on the totals; have is written only when the stream is dropped
TRK_HD int verify_decide(int h_s, int n_s, int n_in, int n_fg, double I, double S, double R, bool use_alpha, int min_fg,
                         int min_samples, double min_support, double min_coverage, double min_iou, int32_t& have) {
  if (n_fg < min_fg) return HRP_VERIFY_UNDECIDED;
  int fail = 0;
  if (min_support >= 0.0 && n_s >= min_samples && !((double)h_s / (double)n_s >= min_support)) fail |= HRP_VERIFY_FAIL_SUPPORT;
  if (min_coverage >= 0.0 && !((double)n_in / (double)n_fg >= min_coverage)) fail |= HRP_VERIFY_FAIL_COVERAGE;
  if (min_iou >= 0.0 && use_alpha && !(I / (S + R - I) >= min_iou)) fail |= HRP_VERIFY_FAIL_IOU;
  if (!fail) return HRP_VERIFY_KEPT;
  have = 0;
  return HRP_VERIFY_DROPPED | fail;
}

// One stream in one thread.  state [nkp][2] float64 is only read; counts [4] = (h_s, n_s, n_in, n_fg), sums [3] = (I, S, R).
TRK_HD int track_verify(const double* state, int nkp, int32_t& have, double sx, double sy, const float* mask, const float* alpha,
                        int hm, int wm, const int32_t (*bones)[2], int nb, int S, double er0, double er1, float min_prob, int min_fg,
                        int min_samples, double min_support, double min_coverage, double min_iou, int32_t* counts, double* sums) {
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  sums[0] = sums[1] = sums[2] = 0.0;
  VerifyGeom g;
  const int early = verify_geometry(state, nkp, have, sx, sy, er0, er1, g);
  if (early) {
    if (early == HRP_VERIFY_DROPPED) have = 0;
    return early;
  }
  int counted = 0, hit = 0;
  for (int s = 0; s < verify_samples(nkp, nb, S); ++s) verify_sample(g, nkp, bones, S, s, mask, hm, wm, min_prob, counted, hit);
  VerifyAcc acc = {0.0, 0.0, 0.0, 0, 0};
  for (int y = 0; y < hm; ++y)
    for (int x = 0; x < wm; ++x) {
      const int64_t i = (int64_t)y * wm + x;
      verify_pixel(g, mask[i], alpha ? alpha[i] : 0.f, alpha != nullptr, x, y, min_prob, acc);
    }
  counts[0] = hit, counts[1] = counted, counts[2] = acc.n_in, counts[3] = acc.n_fg;
  sums[0] = acc.I, sums[1] = acc.S, sums[2] = acc.R;
  return verify_decide(hit, counted, acc.n_in, acc.n_fg, acc.I, acc.S, acc.R, alpha != nullptr, min_fg, min_samples, min_support,
                       min_coverage, min_iou, have);
}

}  // namespace track
