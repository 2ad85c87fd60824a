// Streaming pose tracker: this frame's crop from the last frame's estimate, on the device (the arithmetic is track_core.h).
// Replaces, fed the predicted key-points, the reference loader's per-sample geometry and crop
//   lib/dataset/dream.py:171-216, 287-394; lib/dataset/roboutils.py:59-156, 224-257; lib/utils/geometries.py:360-395
// and the k_values of the step, lib/core/function.py:43-48, 88-98.
//
// hrp_track_prepare is ONE launch: at B = 1 .. 16 the work is latency-bound, so every workgroup derives its stream's record
// itself (lane 0, a few hundred float64 operations, into LDS) instead of waiting for a geometry launch, and then walks its share
// of the pixels of both views.  hrp_track_update and hrp_track_seed (acquisition from a detector's key-points) are one launch with
// one lane per stream.
#include "hrp_common.h"
#include "track_core.h"

static_assert(sizeof(hrp_track_geom) == 112, "hrp_track_geom layout is mirrored by _native.TrackGeom");

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

bool size_ok(int v) { return v >= 1 && v <= HRP_TRACK_MAX_SIZE; }

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
