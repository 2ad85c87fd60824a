// DREAM dataset per-pixel augmentation and crop / resize (reference lib/dataset/dream.py:226-255, roboutils.py:128-195,
// augmentations.py:96-242).  The host draws every random number and does the geometry; these two launches do the pixel work of
// a whole batch from a table of hrp_dream_sample descriptors.  Pillow's and torch's CPU arithmetic is reproduced operation by
// operation (no contraction except where torch's own CPU kernel contracts), so the bytes equal the reference's.
#include "hrp_common.h"

static_assert(sizeof(hrp_dream_sample) == 144, "hrp_dream_sample layout is mirrored by _native.DreamSample");

namespace hrp {
namespace {

constexpr int DREAM_THREADS = 256;

enum : int {
  F_JITTER = HRP_DREAM_JITTER, F_OCCL = HRP_DREAM_OCCLUSION, F_SHARP = HRP_DREAM_SHARPNESS,
  F_CONTRAST = HRP_DREAM_CONTRAST, F_BRIGHT = HRP_DREAM_BRIGHTNESS, F_COLOR = HRP_DREAM_COLOR
};

// Image.blend(degenerate, image, alpha): in1 + alpha * (in2 - in1) in fp32 (alpha is a C float); truncated inside [0, 1],
// clipped to [0, 255] outside it (Pillow Blend.c, pinned against Pillow by tests/test_dream_host.py)
__device__ __forceinline__ int pil_blend(int in1, int in2, float a) {
  const float t = __fadd_rn((float)in1, __fmul_rn(a, (float)(in2 - in1)));
  if (a >= 0.f && a <= 1.f) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// convert("L"): ITU-R 601-2 luma in 16-bit fixed point, rounded
__device__ __forceinline__ int pil_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// np.clip(uint8 * f64, 0, 255) assigned to uint8: truncation toward zero
__device__ __forceinline__ int jitter(int v, double f) {
  double t = __dmul_rn((double)v, f);
  t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
  return (int)t;
}

// channel c of working-frame pixel (x, y) after truncation padding, colour jitter and the occlusion fill (dream.py:226-245)
__device__ __forceinline__ int pre_px(const uint8_t* __restrict__ frame, int H, int W, const hrp_dream_sample& d,
                                      const uint8_t* __restrict__ noise, int x, int y, int c) {
  if ((d.flags & F_OCCL) && x >= d.occ_x && x < d.occ_x + d.occ_w && y >= d.occ_y && y < d.occ_y + d.occ_h)
    return noise[d.noise_off + ((int64_t)(y - d.occ_y) * d.occ_w + (x - d.occ_x)) * 3 + c];
  const int fx = x - d.pad_x, fy = y - d.pad_y;
  if (fx < 0 || fy < 0 || fx >= W || fy >= H) return 0;
  const int v = frame[((int64_t)fy * W + fx) * 3 + c];
  return (d.flags & F_JITTER) ? jitter(v, d.jitter[c]) : v;
}

__device__ __forceinline__ bool desc_ok(const hrp_dream_sample& d, int max_h, int max_w, int64_t noise_bytes, int64_t scratch_bytes) {
  if (d.work_w < 1 || d.work_h < 1 || d.work_w > max_w || d.work_h > max_h) return false;
  if (d.scratch_off < 0 || d.scratch_off + (int64_t)d.work_w * d.work_h * 3 > scratch_bytes) return false;
  if (d.flags & F_OCCL) {
    if (d.occ_x < 0 || d.occ_y < 0 || d.occ_w < 0 || d.occ_h < 0) return false;
    if (d.noise_off < 0 || d.noise_off + (int64_t)d.occ_w * d.occ_h * 3 > noise_bytes) return false;
  }
  return true;
}

// One workgroup per (band of rows, sample).  Writes the working frame after jitter, occlusion and Sharpness, and the exact sum
// of its convert("L") over the band (the Contrast mean of augmentations.py:96-103 / ImageEnhance.Contrast counts every pixel of
// the working frame).  The band sums are plain per-workgroup stores reduced in a fixed order by the crop kernel.
__global__ void __launch_bounds__(DREAM_THREADS) dream_augment_kernel(const uint8_t* __restrict__ frames, int H, int W,
                                                                      const hrp_dream_sample* __restrict__ table,
                                                                      const uint8_t* __restrict__ noise, int64_t noise_bytes,
                                                                      int max_h, int max_w, uint8_t* __restrict__ scratch,
                                                                      int64_t scratch_bytes, unsigned long long* __restrict__ lsum) {
  const int band = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const hrp_dream_sample d = table[b];
  __shared__ unsigned long long part[DREAM_THREADS / 64];
  unsigned long long acc = 0;
  if (desc_ok(d, max_h, max_w, noise_bytes, scratch_bytes)) {
    const uint8_t* frame = frames + (int64_t)b * H * W * 3;
    uint8_t* out = scratch + d.scratch_off;
    const int Ww = d.work_w, Hw = d.work_h;
    const int rows = (Hw + HRP_DREAM_BANDS - 1) / HRP_DREAM_BANDS;
    const int y0 = band * rows, y1 = min(Hw, y0 + rows);
    const int n = y1 > y0 ? (y1 - y0) * Ww : 0;
    const bool sharp = d.flags & F_SHARP;
    const float fs = (float)d.enh[0];
    for (int i = tid; i < n; i += DREAM_THREADS) {
      const int y = y0 + i / Ww, x = i % Ww;
      int o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int p = pre_px(frame, H, W, d, noise, x, y, c);
        if (!sharp) {
          o[c] = p;
          continue;
        }
        // ImageFilter.SMOOTH (3 x 3, [1 1 1; 1 5 1; 1 1 1] / 13, rounded); the border pixels keep their value
        int sm = p;
        if (x > 0 && y > 0 && x < Ww - 1 && y < Hw - 1) {
          int s = 4 * p + 6;
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) s += (dx == 0 && dy == 0) ? p : pre_px(frame, H, W, d, noise, x + dx, y + dy, c);
          sm = s / 13;
        }
        o[c] = pil_blend(sm, p, fs);
      }
      uint8_t* q = out + ((int64_t)y * Ww + x) * 3;
      q[0] = (uint8_t)o[0];
      q[1] = (uint8_t)o[1];
      q[2] = (uint8_t)o[2];
      acc += (unsigned long long)pil_luma(o[0], o[1], o[2]);
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < DREAM_THREADS / 64; ++w) s += part[w];
    lsum[(int64_t)b * HRP_DREAM_BANDS + band] = s;
  }
}

// the pointwise tail of augmentations.py:96-123 on one working-frame pixel: Contrast (mean grey), Brightness, Color
__device__ __forceinline__ void tail(int* v, const hrp_dream_sample& d, int mean) {
  if (d.flags & F_CONTRAST) {
    const float a = (float)d.enh[1];
    for (int c = 0; c < 3; ++c) v[c] = pil_blend(mean, v[c], a);
  }
  if (d.flags & F_BRIGHT) {
    const float a = (float)d.enh[2];
    for (int c = 0; c < 3; ++c) v[c] = pil_blend(0, v[c], a);
  }
  if (d.flags & F_COLOR) {
    const float a = (float)d.enh[3];
    const int l = pil_luma(v[0], v[1], v[2]);
    for (int c = 0; c < 3; ++c) v[c] = pil_blend(l, v[c], a);
  }
}

// canvas pixel (cx, cy) of resize_image's zero-padded S x S square, with the tail applied to the pixels taken from the frame
__device__ __forceinline__ void canvas_px(const uint8_t* __restrict__ work, const hrp_dream_sample& d, int mean, int cx, int cy,
                                          int* v) {
  const int x = cx - d.off_x + d.crop_x0, y = cy - d.off_y + d.crop_y0;
  if (x < d.crop_x0 || x >= d.crop_x1 || y < d.crop_y0 || y >= d.crop_y1 || x < 0 || y < 0 || x >= d.work_w || y >= d.work_h) {
    v[0] = v[1] = v[2] = 0;
    return;
  }
  const uint8_t* p = work + ((int64_t)y * d.work_w + x) * 3;
  v[0] = p[0];
  v[1] = p[1];
  v[2] = p[2];
  tail(v, d, mean);
}

// torch's CPU bilinear source index (align_corners=False): area_pixel_compute_source_index + guard_index_and_lambda
__device__ __forceinline__ void src_index(int o, int in_size, float scale, int& i0, int& i1, float& l0, float& l1) {
  float r = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)o, 0.5f)), 0.5f);
  r = r < 0.f ? 0.f : r;
  i0 = min((int)floorf(r), in_size - 1);
  l1 = __fsub_rn(r, (float)i0);
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l0 = __fsub_rn(1.f, l1);
}

__device__ __forceinline__ float u8f(int v) { return __fdiv_rn((float)v, 255.f); }

// One thread per output pixel of one view: CropResizeToAspectAugmentation's F.interpolate(bilinear) of (canvas / 255), then
// (x * 255).to(uint8), written NCHW.  When S equals the output size the reference returns the canvas unchanged
// (augmentations.py:176-178): copied.
__global__ void __launch_bounds__(DREAM_THREADS) dream_crop_resize_kernel(const uint8_t* __restrict__ scratch,
                                                                          const hrp_dream_sample* __restrict__ table,
                                                                          const unsigned long long* __restrict__ lsum, int max_h,
                                                                          int max_w, int64_t scratch_bytes, uint8_t* __restrict__ out0,
                                                                          int h0, int w0, uint8_t* __restrict__ out1, int h1, int w1) {
  const int b = blockIdx.z, view = blockIdx.y;
  const int h = view ? h1 : h0, w = view ? w1 : w0;
  uint8_t* out = view ? out1 : out0;
  const int i = blockIdx.x * DREAM_THREADS + threadIdx.x;
  if (i >= h * w) return;
  const int oy = i / w, ox = i % w;
  const hrp_dream_sample d = table[b];
  const int64_t plane = (int64_t)h * w;
  uint8_t* q = out + (int64_t)b * 3 * plane + i;
  if (!desc_ok(d, max_h, max_w, INT64_MAX, scratch_bytes) || d.side < 1) {  // the noise was checked by the augment launch
    q[0] = q[plane] = q[2 * plane] = 0;
    return;
  }
  int mean = 0;
  if (d.flags & F_CONTRAST) {  // int(sum / pixels + 0.5), the sum over the bands in band order
    unsigned long long s = 0;
    for (int k = 0; k < HRP_DREAM_BANDS; ++k) s += lsum[(int64_t)b * HRP_DREAM_BANDS + k];
    mean = (int)__dadd_rn(__ddiv_rn((double)s, (double)((int64_t)d.work_w * d.work_h)), 0.5);
  }
  const uint8_t* work = scratch + d.scratch_off;
  const int S = d.side;
  int r[3];
  if (S == h && S == w) {
    canvas_px(work, d, mean, ox, oy, r);
  } else {
    const float sy = __fdiv_rn((float)S, (float)h), sx = __fdiv_rn((float)S, (float)w);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(oy, S, sy, y0, y1, ly0, ly1);
    src_index(ox, S, sx, x0, x1, lx0, lx1);
    int v00[3], v01[3], v10[3], v11[3];
    canvas_px(work, d, mean, x0, y0, v00);
    canvas_px(work, d, mean, x1, y0, v01);
    canvas_px(work, d, mean, x0, y1, v10);
    canvas_px(work, d, mean, x1, y1, v11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // torch's generic CPU kernel (Interpolate<n, scalar_t, index_t, 2>): t0 * w0 + t1 * w1 per dimension, which its build
      // contracts to fma(t0, w0, t1 * w1); pinned against torch by tests/test_dream_host.py
      const float t0 = __fmaf_rn(u8f(v00[c]), lx0, __fmul_rn(u8f(v01[c]), lx1));
      const float t1 = __fmaf_rn(u8f(v10[c]), lx0, __fmul_rn(u8f(v11[c]), lx1));
      const float o = __fmaf_rn(t0, ly0, __fmul_rn(t1, ly1));
      const float s = __fmul_rn(o, 255.f);
      r[c] = s <= 0.f ? 0 : (s >= 255.f ? 255 : (int)s);
    }
  }
  q[0] = (uint8_t)r[0];
  q[plane] = (uint8_t)r[1];
  q[2 * plane] = (uint8_t)r[2];
}

}  // namespace
}  // namespace hrp

using namespace hrp;

extern "C" int hrp_dream_augment(const uint8_t* frames, int B, int H, int W, const hrp_dream_sample* table_dev, const uint8_t* noise,
                                 int64_t noise_bytes, int max_h, int max_w, uint8_t* scratch, int64_t scratch_bytes, uint64_t* lsum,
                                 void* stream) {
  HRP_REQUIRE(frames && table_dev && scratch && lsum && B > 0 && H > 0 && W > 0, "dream_augment: bad args");
  HRP_REQUIRE(max_h >= H && max_w >= W, "dream_augment: working frame bound %d x %d below the frame %d x %d", max_h, max_w, H, W);
  HRP_REQUIRE(noise || noise_bytes == 0, "dream_augment: noise bytes without a buffer");
  hipLaunchKernelGGL(dream_augment_kernel, dim3(HRP_DREAM_BANDS, B), dim3(DREAM_THREADS), 0, (hipStream_t)stream, frames, H, W,
                     table_dev, noise, noise_bytes, max_h, max_w, scratch, scratch_bytes, (unsigned long long*)lsum);
  return check_launch("dream_augment");
}

extern "C" int hrp_dream_crop_resize(const uint8_t* scratch, int64_t scratch_bytes, const hrp_dream_sample* table_dev,
                                     const uint64_t* lsum, int B, int max_h, int max_w, uint8_t* out0, int h0, int w0, uint8_t* out1,
                                     int h1, int w1, void* stream) {
  HRP_REQUIRE(scratch && table_dev && lsum && out0 && B > 0 && h0 > 0 && w0 > 0, "dream_crop_resize: bad args");
  HRP_REQUIRE(!out1 || (h1 > 0 && w1 > 0), "dream_crop_resize: second view %d x %d", h1, w1);
  HRP_REQUIRE(h0 <= 4096 && w0 <= 4096 && h1 <= 4096 && w1 <= 4096, "dream_crop_resize: output larger than 4096");
  const int n = out1 ? max(h0 * w0, h1 * w1) : h0 * w0;
  hipLaunchKernelGGL(dream_crop_resize_kernel, dim3(cdiv(n, DREAM_THREADS), out1 ? 2 : 1, B), dim3(DREAM_THREADS), 0,
                     (hipStream_t)stream, scratch, table_dev, (const unsigned long long*)lsum, max_h, max_w, scratch_bytes, out0, h0,
                     w0, out1, h1, w1);
  return check_launch("dream_crop_resize");
}
