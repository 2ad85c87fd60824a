// Validation metrics of one batch in one launch (hrp_eval_batch, include/hrp.h).
//
// Restates reference lib/core/function.py:137-179: compute_metrics_batch (lib/utils/metrics.py:36-113) for the FK key-points
// and for the integral key-points, and the mean geodesic distance between the predicted and the true base rotation
// (lib/utils/geometries.py:154-162).  The reference does this with ~130 small numpy / torch operations and a device-to-host
// copy of every prediction per batch; here the results land in device arrays that hold the whole epoch.
//
// One workgroup of 256 threads walks the batch in chunks of EV_CH samples:
//   1. one thread per (sample, key-point) writes that pair's nine scalars to LDS; |gt - pred| of the joints and the rotation
//      angle of each sample go to LDS as well;
//   2. thread s adds sample s's key-points in key-point order -> the per-image outputs;
//      thread 255 - c owns column c of the per-batch outputs and adds the chunk's samples to its register in sample order.
// The per-batch sums therefore run over b = 0 .. B-1 in order whatever B is; nothing is reduced across threads.
#include "hrp_common.h"

namespace hrp {

constexpr int EV_CH = 64;                      // samples per chunk
enum { Q_E3 = 0, Q_E2, Q_REL, Q_E3REL, Q_E3I, Q_E2I, Q_RELI, Q_E3RELI, Q_VALID, Q_N };

// rows x, y, z of the rotation matrix (geometries.py:100-115 for the 6-D form, :21-41 for the quaternion)
__device__ __forceinline__ void eval_rotmat(const float* r, int rot_dim, float* R) {
  if (rot_dim == 6) {
    const float na = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    const float x0 = r[0] / na, x1 = r[1] / na, x2 = r[2] / na;
    float z0 = x1 * r[5] - x2 * r[4], z1 = x2 * r[3] - x0 * r[5], z2 = x0 * r[4] - x1 * r[3];
    const float nz = sqrtf(z0 * z0 + z1 * z1 + z2 * z2);
    z0 /= nz; z1 /= nz; z2 /= nz;
    R[0] = x0; R[1] = x1; R[2] = x2;
    R[3] = z1 * x2 - z2 * x1; R[4] = z2 * x0 - z0 * x2; R[5] = z0 * x1 - z1 * x0;
    R[6] = z0; R[7] = z1; R[8] = z2;
  } else {
    const float n = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]) + 1e-9f;
    const float w = r[0] / n, x = r[1] / n, y = r[2] / n, z = r[3] / n;
    const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    R[0] = w2 + x2 - y2 - z2; R[1] = 2.f * xy - 2.f * wz; R[2] = 2.f * wy + 2.f * xz;
    R[3] = 2.f * wz + 2.f * xy; R[4] = w2 - x2 + y2 - z2; R[5] = 2.f * yz - 2.f * wx;
    R[6] = 2.f * xz - 2.f * wy; R[7] = 2.f * wx + 2.f * yz; R[8] = w2 - x2 - y2 + z2;
  }
}

// ||p - g||, ||K p / (K p)_z - g2|| of one predicted point (metrics.py:43, 55, 61)
__device__ __forceinline__ void eval_point(const float* Kb, const float* p, const float* g, const float* g2, float& e3, float& e2) {
  const float dx = p[0] - g[0], dy = p[1] - g[1], dz = p[2] - g[2];
  e3 = sqrtf(dx * dx + dy * dy + dz * dz);
  const float h0 = Kb[0] * p[0] + Kb[1] * p[1] + Kb[2] * p[2], h1 = Kb[3] * p[0] + Kb[4] * p[1] + Kb[5] * p[2],
              h2 = Kb[6] * p[0] + Kb[7] * p[1] + Kb[8] * p[2];
  const float du = h0 / h2 - g2[0], dv = h1 / h2 - g2[1];
  e2 = sqrtf(du * du + dv * dv);
}

__global__ __launch_bounds__(256) void eval_batch_kernel(const hrp_eval_desc d) {
  __shared__ float s_q[Q_N][EV_CH * HRP_FK_MAX_KP];
  __shared__ float s_ej[EV_CH * HRP_FK_MAX_JOINTS];
  __shared__ float s_th[EV_CH];
  const int t = threadIdx.x, B = d.B, nkp = d.nkp, dof = d.dof, root = d.root;
  // per-batch columns: [0, 4 nkp) dis3d, dis2d, dis3d_int, dis2d_int; [4 nkp, 4 nkp + dof) l1_jointerror; then rotation_diff
  const int ncol = 4 * nkp + dof + 1, c = 255 - t;
  const int c_which = c / nkp, c_k = c - c_which * nkp;
  float acc = 0.f, cnt = 0.f;
  for (int b0 = 0; b0 < B; b0 += EV_CH) {
    const int ns = min(EV_CH, B - b0);
    __syncthreads();                     // the previous chunk's readers are done with LDS
    for (int i = t; i < ns * nkp; i += 256) {
      const int s = i / nkp, k = i - s * nkp, b = b0 + s;
      const size_t o = (size_t)b * nkp + k, orow = (size_t)b * nkp + root;
      const float* g = d.gt_kp3d + 3 * o;
      const float* g2 = d.gt_kp2d + 2 * o;
      const float* pf = d.pred_kp3d_fk + 3 * o;
      const float* pi = d.pred_kp3d_int + 3 * o;
      float e3, e2, e3i, e2i;
      eval_point(d.K + 9 * (size_t)b, pf, g, g2, e3, e2);
      eval_point(d.K + 9 * (size_t)b, pi, g, g2, e3i, e2i);
      // closed bounds of the fixed 640 x 480 frame (metrics.py:63)
      const float valid = (g2[0] <= 640.0f && g2[0] >= 0.f && g2[1] <= 480.0f && g2[1] >= 0.f) ? 1.f : 0.f;
      // depth relative to the root key-point (metrics.py:98-110)
      const float g_rel = g[2] - d.gt_kp3d[3 * orow + 2];
      const float rel = (pf[2] - d.pred_kp3d_fk[3 * orow + 2]) - g_rel, reli = (pi[2] - d.pred_kp3d_int[3 * orow + 2]) - g_rel;
      const float dx = pf[0] - g[0], dy = pf[1] - g[1], dxi = pi[0] - g[0], dyi = pi[1] - g[1];
      s_q[Q_E3][i] = e3;
      s_q[Q_E2][i] = e2 * valid;
      s_q[Q_REL][i] = fabsf(rel);
      s_q[Q_E3REL][i] = sqrtf(dx * dx + dy * dy + rel * rel);
      s_q[Q_E3I][i] = e3i;
      s_q[Q_E2I][i] = e2i * valid;
      s_q[Q_RELI][i] = fabsf(reli);
      s_q[Q_E3RELI][i] = sqrtf(dxi * dxi + dyi * dyi + reli * reli);
      s_q[Q_VALID][i] = valid;
    }
    for (int i = t; i < ns * dof; i += 256) {          // metrics.py:82, 89-91
      const size_t o = (size_t)b0 * dof + i;
      s_ej[i] = d.pred_joint ? fabsf(d.gt_joint[o] - d.pred_joint[o]) : 0.f;
    }
    if (t >= 192 && t - 192 < ns) {                   // geometries.py:154-162
      const int b = b0 + t - 192;
      float Rp[9], Rg[9];
      eval_rotmat(d.pred_rot + (size_t)b * d.rot_dim, d.rot_dim, Rp);
      eval_rotmat(d.gt_rot + (size_t)b * d.rot_dim, d.rot_dim, Rg);
      float tr = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) tr += Rp[3 * r] * Rg[3 * r] + Rp[3 * r + 1] * Rg[3 * r + 1] + Rp[3 * r + 2] * Rg[3 * r + 2];
      float cs = (tr - 1.f) / 2.f;
      cs = cs > 1.f ? 1.f : (cs < -1.f ? -1.f : cs);  // a NaN stays a NaN, as through torch.min / torch.max
      s_th[t - 192] = acosf(cs);
    }
    __syncthreads();
    if (t < ns) {                                     // per-image outputs (metrics.py:57, 65-67, 85-87, 95, 101, 110)
      const int b = b0 + t;
      float v[Q_N];
#pragma unroll
      for (int q = 0; q < Q_N; ++q) v[q] = 0.f;
      for (int k = 0; k < nkp; ++k) {
#pragma unroll
        for (int q = 0; q < Q_N; ++q) v[q] += s_q[q][t * nkp + k];
      }
      const int nj = dof - (d.drop_last_joint ? 1 : 0);
      float ej = 0.f;
      for (int j = 0; j < nj; ++j) ej += s_ej[t * dof + j];
      const size_t orow = (size_t)b * nkp + root, w = (size_t)d.offset + b;
      d.error3d[w] = v[Q_E3] / (float)nkp;
      d.error2d[w] = v[Q_E2] / v[Q_VALID];            // 0 / 0 = NaN for an image with nothing in frame, as in the reference
      d.mean_jointerror[w] = d.pred_joint ? ej / (float)nj : 0.f;
      d.error_depth[w] = fabsf(d.pred_kp3d_fk[3 * orow + 2] - d.gt_kp3d[3 * orow + 2]);
      d.batch_error_relative[w] = v[Q_REL] / (float)nkp;
      d.error3d_relative[w] = v[Q_E3REL] / (float)nkp;
      d.error3d_int[w] = v[Q_E3I] / (float)nkp;
      d.error2d_int[w] = v[Q_E2I] / v[Q_VALID];
      d.error_depth_int[w] = fabsf(d.pred_kp3d_int[3 * orow + 2] - d.gt_kp3d[3 * orow + 2]);
      d.batch_error_relative_int[w] = v[Q_RELI] / (float)nkp;
      d.error3d_relative_int[w] = v[Q_E3RELI] / (float)nkp;
    }
    if (c < ncol) {                                   // per-batch columns, samples in order
      if (c < 4 * nkp) {
        const float* q = s_q[c_which == 0 ? Q_E3 : c_which == 1 ? Q_E2 : c_which == 2 ? Q_E3I : Q_E2I];
        for (int s = 0; s < ns; ++s) {
          acc += q[s * nkp + c_k];
          cnt += s_q[Q_VALID][s * nkp + c_k];
        }
      } else if (c < 4 * nkp + dof) {
        for (int s = 0; s < ns; ++s) acc += s_ej[s * dof + c - 4 * nkp];
      } else {
        for (int s = 0; s < ns; ++s) acc += s_th[s];
      }
    }
  }
  if (c < ncol) {                                     // metrics.py:71-74, 83; function.py:169-172
    const size_t row = (size_t)d.batch_index;
    if (c < 4 * nkp) {
      float* out = c_which == 0 ? d.dis3d : c_which == 1 ? d.dis2d : c_which == 2 ? d.dis3d_int : d.dis2d_int;
      out[row * nkp + c_k] = (c_which & 1) ? acc / cnt : acc / (float)B;
    } else if (c < 4 * nkp + dof) {
      d.l1_jointerror[row * dof + c - 4 * nkp] = acc / (float)B;
    } else {
      d.rotation_diff[row] = acc / (float)B;
    }
  }
}

}  // namespace hrp

using namespace hrp;

extern "C" int hrp_eval_batch(const hrp_eval_desc* d, void* stream) {
  HRP_REQUIRE(d, "eval_batch: null descriptor");
  HRP_REQUIRE(d->pred_kp3d_fk && d->pred_kp3d_int && d->gt_kp3d && d->gt_kp2d && d->K && d->pred_rot && d->gt_rot,
              "eval_batch: null input");
  HRP_REQUIRE(!d->pred_joint || d->gt_joint, "eval_batch: pred_joint without gt_joint");
  HRP_REQUIRE(d->error3d && d->error2d && d->mean_jointerror && d->error_depth && d->batch_error_relative && d->error3d_relative &&
              d->error3d_int && d->error2d_int && d->error_depth_int && d->batch_error_relative_int && d->error3d_relative_int, "eval_batch: null per-image output");
  HRP_REQUIRE(d->dis3d && d->dis2d && d->dis3d_int && d->dis2d_int && d->l1_jointerror && d->rotation_diff,
              "eval_batch: null per-batch output");
  HRP_REQUIRE(d->B > 0, "eval_batch: B=%d", d->B);
  HRP_REQUIRE(d->nkp > 0 && d->nkp <= HRP_FK_MAX_KP && d->dof > 0 && d->dof <= HRP_FK_MAX_JOINTS, "eval_batch: nkp=%d dof=%d", d->nkp, d->dof);
  HRP_REQUIRE(d->root >= 0 && d->root < d->nkp, "eval_batch: root=%d of %d key-points", d->root, d->nkp);
  HRP_REQUIRE(!d->drop_last_joint || d->dof > 1, "eval_batch: drop_last_joint with dof=%d", d->dof);
  HRP_REQUIRE(d->rot_dim == 4 || d->rot_dim == 6, "eval_batch: rot_dim=%d", d->rot_dim);
  HRP_REQUIRE(d->offset >= 0 && d->capacity > 0 && (int64_t)d->offset + d->B <= (int64_t)d->capacity,
              "eval_batch: images [%d, %d + %d) do not fit the capacity %d", d->offset, d->offset, d->B, d->capacity);
  HRP_REQUIRE(d->batch_index >= 0 && d->batch_index < d->batch_capacity, "eval_batch: batch %d of a capacity of %d", d->batch_index,
              d->batch_capacity);
  hipLaunchKernelGGL(eval_batch_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *d);
  return check_launch("eval_batch");
}
