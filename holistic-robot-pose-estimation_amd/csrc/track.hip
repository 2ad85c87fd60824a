// Streaming pose tracker: this frame's crop from the last frame's estimate, on the device (the arithmetic is track_core.h).
// Replaces, fed the predicted key-points, the reference loader's per-sample geometry and crop
//   lib/dataset/dream.py:171-216, 287-394; lib/dataset/roboutils.py:59-156, 224-257; lib/utils/geometries.py:360-395
// and the k_values of the step, lib/core/function.py:43-48, 88-98.
//
// hrp_track_prepare is ONE launch: at B = 1 .. 16 the work is latency-bound, so every workgroup derives its stream's record
// itself (lane 0, a few hundred float64 operations, into LDS) instead of waiting for a geometry launch, and then walks its share
// of the pixels of both views.  hrp_track_update and hrp_track_seed (acquisition from a detector's key-points) are one launch with
// one lane per stream.  hrp_track_verify (the estimate against the detector's foreground map) is one launch with one workgroup per
// stream.
#include "hrp_common.h"
#include "track_core.h"

static_assert(sizeof(hrp_track_geom) == 112, "hrp_track_geom layout is mirrored by _native.TrackGeom");
static_assert(sizeof(hrp_track_verify_desc) == 408, "hrp_track_verify_desc layout is mirrored by _native.TrackVerifyDesc");

namespace hrp {
namespace {

constexpr int TRACK_THREADS = 256;
constexpr int TRACK_PX_PER_THREAD = 4;      // pixels a lane writes; every workgroup repeats the geometry, so not one pixel each
constexpr int UPDATE_THREADS = 64;

__global__ void __launch_bounds__(TRACK_THREADS) track_prepare_kernel(
    const uint8_t* __restrict__ frames, const double* __restrict__ state_kp2d, const int32_t* __restrict__ state_have,
    const float* __restrict__ K_original, int H, int W, int nkp, uint8_t* __restrict__ out0, int h0, int w0,
    uint8_t* __restrict__ out1, int h1, int w1, double er0, double er1, int bbox_mode, float* __restrict__ K_root,
    float* __restrict__ K_other, float* __restrict__ k_values, hrp_track_geom* __restrict__ geom) {
  __shared__ hrp_track_geom sg;
  __shared__ float sK[2][9];
  __shared__ float sk;
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) {
    const track::Views vw = {{h0, out1 ? h1 : h0}, {w0, out1 ? w1 : w0}, out1 ? 1 : 0};
    track::track_geometry(state_kp2d + (int64_t)b * nkp * 2, nkp, state_have[b], K_original + b * 9, W, H, vw, er0, er1, bbox_mode, sg,
                          sK[0], sK[1], sk);
  }
  __syncthreads();
  if (blockIdx.x == 0) {                     // the record leaves through the first workgroup of the stream
    if (tid < 9) {
      K_root[b * 9 + tid] = sK[0][tid];
      K_other[b * 9 + tid] = sK[1][tid];
    }
    if (tid == 0) k_values[b] = sk;
    if (tid < (int)(sizeof(hrp_track_geom) / 4)) ((uint32_t*)(geom + b))[tid] = ((const uint32_t*)&sg)[tid];
  }
  const hrp_track_geom g = sg;
  const uint8_t* frame = frames + (int64_t)b * H * W * 3;
  const int n0 = h0 * w0, n1 = out1 ? h1 * w1 : 0;
  for (int i = blockIdx.x * TRACK_THREADS + tid; i < n0 + n1; i += gridDim.x * TRACK_THREADS) {
    const int view = i >= n0;
    const int j = view ? i - n0 : i;
    const int h = view ? h1 : h0, w = view ? w1 : w0;
    uint8_t rgb[3];
    track::track_pixel(frame, W, H, g, h, w, j % w, j / w, rgb);
    const int64_t plane = (int64_t)h * w;
    uint8_t* q = (view ? out1 : out0) + (int64_t)b * 3 * plane + j;
    q[0] = rgb[0];
    q[plane] = rgb[1];
    q[2 * plane] = rgb[2];
  }
}

__global__ void __launch_bounds__(UPDATE_THREADS) track_update_kernel(const float* __restrict__ xyz_fk,
                                                                      const float* __restrict__ K_original, int B, int nkp, int W,
                                                                      int H, int min_inside, double* __restrict__ state_kp2d,
                                                                      int32_t* __restrict__ state_have, float* __restrict__ kp2d_out,
                                                                      int32_t* __restrict__ status) {
  const int b = blockIdx.x * UPDATE_THREADS + threadIdx.x;
  if (b >= B) return;
  const int have = track::track_update(xyz_fk + (int64_t)b * nkp * 3, nkp, K_original + b * 9, W, H, min_inside,
                                       state_kp2d + (int64_t)b * nkp * 2, kp2d_out + (int64_t)b * nkp * 2);
  state_have[b] = have;
  if (!have) status[b] |= HRP_TRACK_LOST_OUT;
}

__global__ void __launch_bounds__(UPDATE_THREADS) track_seed_kernel(const float* __restrict__ det_kp, int B, int nkp, double inv_sx,
                                                                    double inv_sy, const float* __restrict__ mask, int hm, int wm,
                                                                    float min_prob, const float* __restrict__ ms, float min_peak,
                                                                    int min_inside, int force, int W, int H,
                                                                    double* __restrict__ state_kp2d, int32_t* __restrict__ state_have,
                                                                    int32_t* __restrict__ seed_status) {
  const int b = blockIdx.x * UPDATE_THREADS + threadIdx.x;
  if (b >= B) return;
  int32_t have = state_have[b];
  const int st = track::track_seed(det_kp + (int64_t)b * nkp * 2, nkp, inv_sx, inv_sy, mask ? mask + (int64_t)b * hm * wm : nullptr, hm,
                                   wm, min_prob, ms ? ms + (int64_t)b * nkp * 2 : nullptr, min_peak, min_inside, force, W, H,
                                   state_kp2d + (int64_t)b * nkp * 2, have);
  if (st == HRP_SEED_TAKEN) state_have[b] = have;
  seed_status[b] = st;
}

// ---- verification ---------------------------------------------------------------------------------------------------------------
// One workgroup per stream.  Lane 0 derives the key-points in detector pixels and the box into LDS; the lanes then share out the
// sample points and the pixels.  The map of a stream is hm * wm contiguous floats, so it is walked flat: scalar loads up to the
// first 16-byte boundary, float4 loads (four vectors of a lane in flight) from there, a scalar tail; a silhouette whose
// alignment differs from the mask's makes the whole walk scalar.  Lane sums are folded by shuffles within a wave and by lane 0
// over the four waves, always in the same order.
constexpr int VERIFY_THREADS = 256;
constexpr int VERIFY_WAVES = VERIFY_THREADS / 64;
constexpr int VERIFY_UNROLL = 4;

template <typename T>
__device__ inline T verify_wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(VERIFY_THREADS) track_verify_kernel(const hrp_track_verify_desc d) {
  __shared__ track::VerifyGeom sg;
  __shared__ int32_t sbones[HRP_TRACK_MAX_BONES][2];
  __shared__ int s_early;
  __shared__ double sred[3][VERIFY_WAVES];
  __shared__ int sredi[4][VERIFY_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nkp = d.nkp, hm = d.hm, wm = d.wm;
  if (tid == 0)
    s_early = track::verify_geometry(d.state_kp2d + (int64_t)b * nkp * 2, nkp, d.state_have[b], d.scale[0], d.scale[1], d.extend_ratio[0],
                                     d.extend_ratio[1], sg);
  if (tid < d.nb) {
    sbones[tid][0] = d.bones[tid][0];
    sbones[tid][1] = d.bones[tid][1];
  }
  __syncthreads();
  const int early = s_early;
  if (early) {                               // skipped, or dropped for a state that is not finite: zero counts and sums
    if (tid == 0) {
      d.verify_status[b] = early;
      if (early == HRP_VERIFY_DROPPED) d.state_have[b] = 0;
    }
    if (tid < 4) d.counts[b * 4 + tid] = 0;
    if (tid < 3) d.sums[b * 3 + tid] = 0.0;
    return;
  }
  const int n = hm * wm;                     // <= 4096 * 4096
  const float* mask = d.mask + (int64_t)b * n;
  const float* alpha = d.alpha ? d.alpha + (int64_t)b * n : nullptr;
  const bool use_alpha = alpha != nullptr;
  const float min_prob = d.min_prob;

  int counted = 0, hit = 0;
  const int ns = track::verify_samples(nkp, d.nb, d.samples);
  for (int s = tid; s < ns; s += VERIFY_THREADS) track::verify_sample(sg, nkp, sbones, d.samples, s, mask, hm, wm, min_prob, counted, hit);

  track::VerifyAcc acc = {0.0, 0.0, 0.0, 0, 0};
  const int mis = (int)(((uintptr_t)mask >> 2) & 3);
  const bool vec = !use_alpha || (int)(((uintptr_t)alpha >> 2) & 3) == mis;
  const int head = vec ? track::imin(n, (4 - mis) & 3) : n;
  const int nvec = (n - head) / 4, tail0 = head + 4 * nvec;
  for (int i = tid; i < head + (n - tail0); i += VERIFY_THREADS) {
    const int p = i < head ? i : tail0 + (i - head);
    if (p >= 0 && p < n) track::verify_pixel(sg, mask[p], use_alpha ? alpha[p] : 0.f, use_alpha, p % wm, p / wm, min_prob, acc);
  }
  for (int v0 = tid; v0 < nvec; v0 += VERIFY_THREADS * VERIFY_UNROLL) {
    float4 m4[VERIFY_UNROLL], a4[VERIFY_UNROLL];
#pragma unroll
    for (int u = 0; u < VERIFY_UNROLL; ++u) {
      const int v = v0 + u * VERIFY_THREADS;
      m4[u] = a4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (v < nvec) {
        m4[u] = *reinterpret_cast<const float4*>(mask + head + 4 * v);
        if (use_alpha) a4[u] = *reinterpret_cast<const float4*>(alpha + head + 4 * v);
      }
    }
#pragma unroll
    for (int u = 0; u < VERIFY_UNROLL; ++u) {
      const int v = v0 + u * VERIFY_THREADS;
      if (v >= nvec) break;
      const int p = head + 4 * v;
      int x = p % wm, y = p / wm;
      const float mm[4] = {m4[u].x, m4[u].y, m4[u].z, m4[u].w}, aa[4] = {a4[u].x, a4[u].y, a4[u].z, a4[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        track::verify_pixel(sg, mm[k], aa[k], use_alpha, x, y, min_prob, acc);
        if (++x == wm) {
          x = 0;
          ++y;
        }
      }
    }
  }

  const double wI = verify_wave_sum(acc.I), wS = verify_wave_sum(acc.S), wR = verify_wave_sum(acc.R);
  const int wh = verify_wave_sum(hit), wc = verify_wave_sum(counted), win = verify_wave_sum(acc.n_in), wfg = verify_wave_sum(acc.n_fg);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    sred[0][w] = wI, sred[1][w] = wS, sred[2][w] = wR;
    sredi[0][w] = wh, sredi[1][w] = wc, sredi[2][w] = win, sredi[3][w] = wfg;
  }
  __syncthreads();
  if (tid == 0) {
    double s[3];
    int c[4];
    for (int q = 0; q < 3; ++q) {
      s[q] = sred[q][0];
      for (int w = 1; w < VERIFY_WAVES; ++w) s[q] += sred[q][w];
    }
    for (int q = 0; q < 4; ++q) {
      c[q] = sredi[q][0];
      for (int w = 1; w < VERIFY_WAVES; ++w) c[q] += sredi[q][w];
    }
    int32_t have = 1;
    const int st = track::verify_decide(c[0], c[1], c[2], c[3], s[0], s[1], s[2], use_alpha, d.min_fg, d.min_samples, d.min_support,
                                        d.min_coverage, d.min_iou, have);
    if (!have) d.state_have[b] = 0;
    d.verify_status[b] = st;
    for (int q = 0; q < 4; ++q) d.counts[b * 4 + q] = c[q];
    for (int q = 0; q < 3; ++q) d.sums[b * 3 + q] = s[q];
  }
}

bool size_ok(int v) { return v >= 1 && v <= HRP_TRACK_MAX_SIZE; }
bool threshold_ok(double v) { return v <= 1.0; }               // (false for NaN; a negative value switches the criterion off)

}  // namespace
}  // namespace hrp

using namespace hrp;

extern "C" int hrp_track_prepare(const uint8_t* frames, const double* state_kp2d, const int32_t* state_have, const float* K_original,
                                 int B, int H, int W, int nkp, uint8_t* out_root, int h0, int w0, uint8_t* out_other, int h1, int w1,
                                 const double* extend_ratio, int bbox_mode, float* K_root, float* K_other, float* k_values,
                                 hrp_track_geom* geom, void* stream) {
  HRP_REQUIRE(frames && state_kp2d && state_have && K_original && out_root && extend_ratio && K_root && K_other && k_values && geom,
              "track_prepare: null pointer");
  HRP_REQUIRE(B >= 1 && B <= 65535, "track_prepare: %d streams", B);
  HRP_REQUIRE(nkp >= 1 && nkp <= HRP_TRACK_MAX_KP, "track_prepare: %d key-points, want 1 .. %d", nkp, HRP_TRACK_MAX_KP);
  HRP_REQUIRE(size_ok(H) && size_ok(W), "track_prepare: frame %d x %d, want 1 .. %d", H, W, HRP_TRACK_MAX_SIZE);
  HRP_REQUIRE(size_ok(h0) && size_ok(w0), "track_prepare: root view %d x %d, want 1 .. %d", h0, w0, HRP_TRACK_MAX_SIZE);
  HRP_REQUIRE(!out_other || (size_ok(h1) && size_ok(w1)), "track_prepare: other view %d x %d, want 1 .. %d", h1, w1, HRP_TRACK_MAX_SIZE);
  HRP_REQUIRE(bbox_mode == HRP_TRACK_BBOX_EXTENDED || bbox_mode == HRP_TRACK_BBOX_ORIGIN || bbox_mode == HRP_TRACK_BBOX_STRICT,
              "track_prepare: bbox_mode %d", bbox_mode);
  const int n = h0 * w0 + (out_other ? h1 * w1 : 0);
  hipLaunchKernelGGL(track_prepare_kernel, dim3(cdiv(n, TRACK_THREADS * TRACK_PX_PER_THREAD), B), dim3(TRACK_THREADS), 0,
                     (hipStream_t)stream, frames, state_kp2d, state_have, K_original, H, W, nkp, out_root, h0, w0, out_other, h1, w1,
                     extend_ratio[0], extend_ratio[1], bbox_mode, K_root, K_other, k_values, geom);
  return check_launch("track_prepare");
}

extern "C" int hrp_track_update(const float* xyz_fk, const float* K_original, int B, int nkp, int W, int H, int min_inside,
                                double* state_kp2d, int32_t* state_have, float* kp2d_out, int32_t* status, void* stream) {
  HRP_REQUIRE(xyz_fk && K_original && state_kp2d && state_have && kp2d_out && status, "track_update: null pointer");
  HRP_REQUIRE(B >= 1 && B <= 65535, "track_update: %d streams", B);
  HRP_REQUIRE(nkp >= 1 && nkp <= HRP_TRACK_MAX_KP, "track_update: %d key-points, want 1 .. %d", nkp, HRP_TRACK_MAX_KP);
  HRP_REQUIRE(size_ok(H) && size_ok(W), "track_update: frame %d x %d, want 1 .. %d", H, W, HRP_TRACK_MAX_SIZE);
  hipLaunchKernelGGL(track_update_kernel, dim3(cdiv(B, UPDATE_THREADS)), dim3(UPDATE_THREADS), 0, (hipStream_t)stream, xyz_fk,
                     K_original, B, nkp, W, H, min_inside, state_kp2d, state_have, kp2d_out, status);
  return check_launch("track_update");
}

extern "C" int hrp_track_seed(const float* det_kp, int B, int nkp, const double* inv_scale, const float* mask, int hm, int wm,
                              float min_prob, const float* ms, float min_peak, int min_inside, int force, int W, int H,
                              double* state_kp2d, int32_t* state_have, int32_t* seed_status, void* stream) {
  HRP_REQUIRE(det_kp && inv_scale && state_kp2d && state_have && seed_status, "track_seed: null pointer");
  HRP_REQUIRE(B >= 1 && B <= 65535, "track_seed: %d streams", B);
  HRP_REQUIRE(nkp >= 1 && nkp <= HRP_TRACK_MAX_KP, "track_seed: %d key-points, want 1 .. %d", nkp, HRP_TRACK_MAX_KP);
  HRP_REQUIRE(size_ok(H) && size_ok(W), "track_seed: frame %d x %d, want 1 .. %d", H, W, HRP_TRACK_MAX_SIZE);
  HRP_REQUIRE(!mask || (size_ok(hm) && size_ok(wm)), "track_seed: mask %d x %d, want 1 .. %d", hm, wm, HRP_TRACK_MAX_SIZE);
  HRP_REQUIRE(track::finite64(inv_scale[0]) && track::finite64(inv_scale[1]) && inv_scale[0] > 0.0 && inv_scale[1] > 0.0,
              "track_seed: inv_scale must be finite and positive");
  hipLaunchKernelGGL(track_seed_kernel, dim3(cdiv(B, UPDATE_THREADS)), dim3(UPDATE_THREADS), 0, (hipStream_t)stream, det_kp, B, nkp,
                     inv_scale[0], inv_scale[1], mask, hm, wm, min_prob, ms, min_peak, min_inside, force, W, H, state_kp2d, state_have,
                     seed_status);
  return check_launch("track_seed");
}

extern "C" int hrp_track_verify(const hrp_track_verify_desc* d, void* stream) {
  HRP_REQUIRE(d && d->state_kp2d && d->state_have && d->mask && d->verify_status && d->counts && d->sums, "track_verify: null pointer");
  HRP_REQUIRE(((uintptr_t)d->mask & 3) == 0 && ((uintptr_t)d->alpha & 3) == 0 && ((uintptr_t)d->state_kp2d & 7) == 0 &&
                  ((uintptr_t)d->sums & 7) == 0, "track_verify: a buffer is not aligned to its element size");
  HRP_REQUIRE(d->B >= 1 && d->B <= 65535, "track_verify: %d streams", d->B);
  HRP_REQUIRE(d->nkp >= 1 && d->nkp <= HRP_TRACK_MAX_KP, "track_verify: %d key-points, want 1 .. %d", d->nkp, HRP_TRACK_MAX_KP);
  HRP_REQUIRE(size_ok(d->hm) && size_ok(d->wm), "track_verify: mask %d x %d, want 1 .. %d", d->hm, d->wm, HRP_TRACK_MAX_SIZE);
  HRP_REQUIRE(d->nb >= 0 && d->nb <= HRP_TRACK_MAX_BONES, "track_verify: %d bones, want 0 .. %d", d->nb, HRP_TRACK_MAX_BONES);
  for (int i = 0; i < d->nb; ++i)
    HRP_REQUIRE(d->bones[i][0] >= 0 && d->bones[i][0] < d->nkp && d->bones[i][1] >= 0 && d->bones[i][1] < d->nkp,
                "track_verify: bone %d joins key-points %d and %d of %d", i, d->bones[i][0], d->bones[i][1], d->nkp);
  HRP_REQUIRE(d->samples >= 1 && d->samples <= HRP_TRACK_MAX_SAMPLES, "track_verify: %d samples per bone, want 1 .. %d", d->samples,
              HRP_TRACK_MAX_SAMPLES);
  HRP_REQUIRE(track::finite64(d->scale[0]) && track::finite64(d->scale[1]) && d->scale[0] > 0.0 && d->scale[1] > 0.0,
              "track_verify: scale must be finite and positive");
  HRP_REQUIRE(track::finite64(d->extend_ratio[0]) && track::finite64(d->extend_ratio[1]), "track_verify: extend_ratio must be finite");
  HRP_REQUIRE(threshold_ok(d->min_support) && threshold_ok(d->min_coverage) && threshold_ok(d->min_iou),
              "track_verify: thresholds %g, %g, %g, want <= 1 (negative: off)", d->min_support, d->min_coverage, d->min_iou);
  HRP_REQUIRE(!(d->min_iou >= 0.0) || d->alpha, "track_verify: min_iou %g without a silhouette", d->min_iou);
  hipLaunchKernelGGL(track_verify_kernel, dim3(d->B), dim3(VERIFY_THREADS), 0, (hipStream_t)stream, *d);
  return check_launch("track_verify");
}
