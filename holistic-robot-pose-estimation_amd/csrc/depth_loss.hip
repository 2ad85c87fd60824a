// The DepthNet trainer's step after the model call in one launch (hrp_depth_loss, include/hrp.h).
//
// Restates reference scripts/train_depthnet.py:220-268: the mm -> m division of the model output, the depth loss (l1 | mse) in its
// three forms (plain, xy branch, multi_kp), the masked xy loss, and the per-image |depth|, |x|, |y| errors that validate (:276-303)
// copies to the host per batch; here they land in device arrays that hold the whole epoch, next to the batch's loss.  The gradient
// with respect to the model output is written in the same pass (autograd of nn.L1Loss / nn.MSELoss).
//
// One workgroup of 256 threads walks the batch in chunks of DL_CH samples:
//   1. thread s computes sample s: its gradient row, its three errors, and its contributions to the depth sum and to the xy sum,
//      which go to LDS;
//   2. thread 0 adds the chunk's depth contributions to its register in sample order, thread 64 (another wave) the xy ones.
// The sums therefore run over b = 0 .. B-1 in order whatever B is; nothing is reduced across threads and there are no atomics.
//
// The xy branch's depth term keeps the reference's shapes: coord[:, 2] / 1000 is [B], gt_root_depth is [B, 1], and torch broadcasts
// the pair to [B, B] (:223, :250) - the mean over every pair (prediction j, target i).  Thread j walks the targets in order.
#include "hrp_common.h"

namespace hrp {

constexpr int DL_CH = 256;                     // samples per chunk: one per thread

template <bool MSE>
__device__ __forceinline__ void dl_term(float e, float& value, float& slope) {
  if (MSE) {
    value = e * e;
    slope = 2.f * e;
  } else {
    value = fabsf(e);
    slope = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);   // torch.sign: sign(0) = 0 (a NaN gives 0 here, NaN in the loss)
  }
}

template <bool MSE>
__device__ __forceinline__ float dl_sample(const hrp_depth_loss_desc& d, int b, float n_d, float* __restrict__ g_row) {
  const float* p = d.pred + (size_t)b * d.W;
  float sum = 0.f, v, s;
  if (d.nk > 0) {                                                        // :226-227, 263-266
    const float* g = d.gt_kp3d + (size_t)b * d.J * 3;
    for (int k = 0; k < d.nk; ++k) {
      dl_term<MSE>(p[k] / 1000.0f - g[3 * d.kp_index[k] + 2], v, s);
      sum += v;
      if (g_row) g_row[k] = s / n_d / 1000.0f;
    }
  } else if (d.xy_loss != HRP_XY_LOSS_NONE) {                            // :223, 250-252: [B] against [B, 1]
    const float pr = p[2] / 1000.0f;
    float slope = 0.f;
    for (int i = 0; i < d.B; ++i) {
      dl_term<MSE>(pr - d.gt_root_trans[3 * (size_t)i + 2], v, s);
      sum += v;
      slope += s;
    }
    if (g_row) g_row[2] = slope / n_d / 1000.0f;
  } else {                                                               // :231-232, 249-252
    dl_term<MSE>(p[0] / 1000.0f - d.gt_root_trans[3 * (size_t)b + 2], v, s);
    sum = v;
    if (g_row) g_row[0] = s / n_d / 1000.0f;
  }
  return sum;
}

__global__ __launch_bounds__(256) void depth_loss_kernel(const hrp_depth_loss_desc d) {
  __shared__ float s_d[DL_CH];
  __shared__ float s_xy[DL_CH];
  __shared__ float s_total_xy;
  const int t = threadIdx.x, B = d.B, W = d.W;
  const bool xy = d.xy_loss != HRP_XY_LOSS_NONE;
  const float n_d = xy ? (float)B * (float)B : (d.nk > 0 ? (float)B * (float)d.nk : (float)B);
  const float n_xy = 2.f * (float)B;
  float acc = 0.f;                               // thread 0: depth sum; thread 64: xy sum
  for (int b0 = 0; b0 < B; b0 += DL_CH) {
    const int ns = min(DL_CH, B - b0);
    __syncthreads();                             // the previous chunk's readers are done with LDS
    if (t < ns) {
      const int b = b0 + t;
      const float* p = d.pred + (size_t)b * W;
      const float* g = d.gt_root_trans + 3 * (size_t)b;
      float* g_row = d.d_pred ? d.d_pred + (size_t)b * W : nullptr;
      s_d[t] = d.depth_loss == HRP_DEPTH_LOSS_MSE ? dl_sample<true>(d, b, n_d, g_row) : dl_sample<false>(d, b, n_d, g_row);
      float cxy = 0.f;
      if (xy) {                                  // :247, 255-259
        const float m = d.mask[b];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float v, s;
          if (d.xy_loss == HRP_XY_LOSS_MSE) dl_term<true>(p[c] * m - g[c] * m, v, s);
          else dl_term<false>(p[c] * m - g[c] * m, v, s);
          cxy += v;
          if (g_row) g_row[c] = s / n_xy * m;
        }
      }
      s_xy[t] = cxy;
      if (d.errors) {                            // :236-241
        const size_t w = (size_t)d.offset + b, cap = (size_t)d.capacity;
        d.errors[w] = fabsf(p[d.root_col] / 1000.0f - g[2]);
        d.errors[cap + w] = xy ? fabsf(p[0] - g[0]) : 0.f;
        d.errors[2 * cap + w] = xy ? fabsf(p[1] - g[1]) : 0.f;
      }
    }
    __syncthreads();
    if (t == 0) {
      for (int s = 0; s < ns; ++s) acc += s_d[s];
    } else if (t == 64 && xy) {
      for (int s = 0; s < ns; ++s) acc += s_xy[s];
    }
  }
  if (t == 64) s_total_xy = acc;
  __syncthreads();
  if (t == 0) {
    float loss = acc / n_d;
    if (xy) loss += s_total_xy / n_xy;           // loss += ... (:257, 259)
    d.loss[0] = loss;
    if (d.errors) d.losses[d.batch_index] = loss;
  }
}

}  // namespace hrp

using namespace hrp;

extern "C" int hrp_depth_loss(const hrp_depth_loss_desc* d, void* stream) {
  HRP_REQUIRE(d, "depth_loss: null descriptor");
  HRP_REQUIRE(d->pred && d->gt_root_trans && d->loss, "depth_loss: null pred, gt_root_trans or loss");
  HRP_REQUIRE(d->B > 0, "depth_loss: B=%d", d->B);
  HRP_REQUIRE(d->depth_loss == HRP_DEPTH_LOSS_L1 || d->depth_loss == HRP_DEPTH_LOSS_MSE, "depth_loss: unknown depth_loss kind %d",
              d->depth_loss);
  HRP_REQUIRE(d->xy_loss == HRP_XY_LOSS_NONE || d->xy_loss == HRP_XY_LOSS_L1 || d->xy_loss == HRP_XY_LOSS_MSE,
              "depth_loss: unknown xy_loss kind %d", d->xy_loss);
  HRP_REQUIRE(d->nk >= 0 && d->nk <= HRP_DEPTH_LOSS_MAX_KP, "depth_loss: nk=%d (at most %d key-points)", d->nk, HRP_DEPTH_LOSS_MAX_KP);
  const bool xy = d->xy_loss != HRP_XY_LOSS_NONE;
  HRP_REQUIRE(!(xy && d->nk > 0), "depth_loss: the xy branch and multi_kp (nk=%d) exclude each other", d->nk);
  const int want_w = d->nk > 0 ? d->nk : (xy ? 3 : 1);
  HRP_REQUIRE(d->W == want_w, "depth_loss: W=%d, this mode (xy_loss %d, nk %d) has W=%d", d->W, d->xy_loss, d->nk, want_w);
  HRP_REQUIRE(d->root_col >= 0 && d->root_col < d->W, "depth_loss: root_col=%d of %d columns", d->root_col, d->W);
  HRP_REQUIRE(!xy || d->root_col == 2, "depth_loss: root_col=%d, the xy branch keeps the depth in column 2", d->root_col);
  if (d->nk > 0) {
    HRP_REQUIRE(d->gt_kp3d, "depth_loss: null gt_kp3d with nk=%d", d->nk);
    for (int k = 0; k < d->nk; ++k)
      HRP_REQUIRE(d->kp_index[k] >= 0 && d->kp_index[k] < d->J, "depth_loss: kp_index[%d]=%d of %d key-points", k, d->kp_index[k], d->J);
  }
  HRP_REQUIRE(!xy || d->mask, "depth_loss: null mask with the xy branch");
  HRP_REQUIRE(!d->want_grad || d->d_pred, "depth_loss: want_grad with a null d_pred");
  if (d->errors) {
    HRP_REQUIRE(d->losses, "depth_loss: null losses with errors");
    HRP_REQUIRE(d->offset >= 0 && d->capacity > 0 && (int64_t)d->offset + d->B <= (int64_t)d->capacity,
                "depth_loss: images [%d, %d + %d) do not fit the capacity %d", d->offset, d->offset, d->B, d->capacity);
    HRP_REQUIRE(d->batch_index >= 0 && d->batch_index < d->batch_capacity, "depth_loss: batch %d of a capacity of %d", d->batch_index,
                d->batch_capacity);
  }
  hrp_depth_loss_desc k = *d;
  if (!k.want_grad) k.d_pred = nullptr;
  hipLaunchKernelGGL(depth_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, k);
  return check_launch("depth_loss");
}
