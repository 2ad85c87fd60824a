// The per-step bookkeeping of the self-supervised trainer in one launch (hrp_sim2real_monitor, include/hrp.h).
//
// Restates reference scripts/train_sim2real.py:313-400: the seven supervised terms the script computes every step for its logs
// (all detached, :396-398) - in THIS script's form, which is not lib/core/function.py's: loss_uv is the plain mean of the root
// key-point error (:350-353), not a masked quotient.  The four mask terms and the loss of hrp_sim2real_loss are copied next to
// them, so that `row` is the twelve numbers the training loop hands to its meters (:649-660) and validate to its own (:558-569);
// the meters themselves (sum and count, AverageValueMeter) live on the device and are advanced here, which is what takes the
// reference's twelve .detach().cpu().numpy() per step out of the loop.
//
// One workgroup of 256 threads walks the batch in chunks of MON_CH = 64 samples; wave w of the workgroup does part w of sample
// `lane` of the chunk:
//   wave 0   sum_k (pose - gt)^2, sum_k (rot - gt)^2                           k in index order
//   wave 1   |depth - gt_z|, ||(root_uv - gt) / S||, e = ||trans - gt||, e exp(-20 e)
//   wave 2   sum_k ||xyz_fk - gt_kp3d||
//   wave 3   sum_k ||proj(K, xyz_fk) / S - gt_kp2d / S|| mask, sum_k (mask != 0)
// The per-sample values go to LDS; thread 64 (c & 3) + (c >> 2) owns column c and adds the chunk's samples to its register in sample
// order.  Every sum therefore runs over k within a sample, then over b = 0 .. B-1, in index order whatever B is; nothing is reduced
// across threads and there are no atomics: the row is bit-reproducible.  Thread 0 then forms the twelve values, decides the
// loss_trans branch (:367) from the finished mean, writes row / rows[row_index] and advances the meters.
#include "hrp_common.h"

namespace hrp {

constexpr int MON_CH = 64;                     // samples per chunk: one per lane
enum { MQ_JOINT = 0, MQ_ROT, MQ_DEPTH, MQ_UV, MQ_E, MQ_EDAMP, MQ_E3, MQ_E2, MQ_NVALID, MQ_N };

__global__ __launch_bounds__(256) void sim2real_monitor_kernel(const hrp_sim2real_monitor_desc d) {
  __shared__ float s_v[MQ_N][MON_CH];
  __shared__ float s_tot[MQ_N];
  const int t = threadIdx.x, part = t >> 6, lane = t & 63;
  const int B = d.B, P = d.P, J = d.J;
  const float S = d.image_size;
  // column c of the per-batch sums belongs to thread 64 (c & 3) + (c >> 2): the nine walks are spread over the four waves
  const int c = lane < 3 ? 4 * lane + part : MQ_N;
  float acc = 0.f;
  for (int b0 = 0; b0 < B; b0 += MON_CH) {
    const int ns = min(MON_CH, B - b0);
    __syncthreads();                             // the previous chunk's readers are done with LDS
    if (lane < ns) {
      const size_t b = (size_t)b0 + lane;
      if (part == 0) {                           // :321-322, 330-331
        float sj = 0.f, sr = 0.f;
        for (int k = 0; k < P; ++k) {
          const float e = d.pose[b * P + k] - d.gt_pose[b * P + k];
          sj += e * e;
        }
        for (int k = 0; k < 6; ++k) {
          const float e = d.rot[b * 6 + k] - d.gt_root_rot[b * 6 + k];
          sr += e * e;
        }
        s_v[MQ_JOINT][lane] = sj;
        s_v[MQ_ROT][lane] = sr;
      } else if (part == 1) {                    // :337-338, 350-353, 363-370
        const float* g = d.gt_root_trans + 3 * b;
        s_v[MQ_DEPTH][lane] = fabsf(d.depth[b] - g[2]);
        const float ux = (d.root_uv[2 * b] - d.gt_root_uv[2 * b]) / S, uy = (d.root_uv[2 * b + 1] - d.gt_root_uv[2 * b + 1]) / S;
        s_v[MQ_UV][lane] = sqrtf(ux * ux + uy * uy);
        const float dx = d.trans[3 * b] - g[0], dy = d.trans[3 * b + 1] - g[1], dz = d.trans[3 * b + 2] - g[2];
        const float e = sqrtf(dx * dx + dy * dy + dz * dz);
        s_v[MQ_E][lane] = e;
        s_v[MQ_EDAMP][lane] = e * expf(-20.0f * e);
      } else if (part == 2) {                    // :374-377
        float s3 = 0.f;
        for (int k = 0; k < J; ++k) {
          const float* p = d.xyz_fk + 3 * (b * J + k);
          const float* g = d.gt_kp3d + 3 * (b * J + k);
          const float ex = p[0] - g[0], ey = p[1] - g[1], ez = p[2] - g[2];
          s3 += sqrtf(ex * ex + ey * ey + ez * ez);
        }
        s_v[MQ_E3][lane] = s3;
      } else {                                   // :243, 381-386; transforms.py:17-21
        const float* Kb = d.K + 9 * b;
        float s2 = 0.f, nv = 0.f;
        for (int k = 0; k < J; ++k) {
          const float* p = d.xyz_fk + 3 * (b * J + k);
          const float* g2 = d.gt_kp2d + 2 * (b * J + k);
          const float m = d.mask[b * J + k];
          const float h0 = Kb[0] * p[0] + Kb[1] * p[1] + Kb[2] * p[2], h1 = Kb[3] * p[0] + Kb[4] * p[1] + Kb[5] * p[2],
                      h2 = Kb[6] * p[0] + Kb[7] * p[1] + Kb[8] * p[2];
          const float qx = (h0 / h2) / S - g2[0] / S, qy = (h1 / h2) / S - g2[1] / S;
          s2 += sqrtf(qx * qx + qy * qy) * m;
          nv += m != 0.f ? 1.f : 0.f;
        }
        s_v[MQ_E2][lane] = s2;
        s_v[MQ_NVALID][lane] = nv;
      }
    }
    __syncthreads();
    if (c < MQ_N) {
      for (int s = 0; s < ns; ++s) acc += s_v[c][s];
    }
  }
  if (c < MQ_N) s_tot[c] = acc;
  __syncthreads();
  if (t == 0) {
    const float fB = (float)B;
    const float mean_e = s_tot[MQ_E] / fB;
    float row[12];
    row[0] = d.mask_terms ? d.mask_terms[0] : 0.f;                    // loss                       (:402, 468)
    row[1] = s_tot[MQ_JOINT] / (fB * (float)P);                        // loss_joint
    row[2] = s_tot[MQ_ROT] / (fB * 6.f);                               // loss_rot
    row[3] = mean_e > 0.5f ? s_tot[MQ_EDAMP] / fB : mean_e;            // loss_trans                 (:366-370)
    row[4] = s_tot[MQ_UV] / fB;                                        // loss_uv
    row[5] = s_tot[MQ_DEPTH] / fB;                                     // loss_depth
    row[6] = s_tot[MQ_E2] / s_tot[MQ_NVALID];                           // loss_error2d: 0 / 0 = NaN as in the reference
    row[7] = s_tot[MQ_E3] / (fB * (float)J);                           // loss_error3d
    row[8] = d.mask_terms ? d.mask_terms[1] : 0.f;                    // loss_mask                  (:399, 463-466)
    row[9] = d.mask_terms ? d.mask_terms[3] : 0.f;                    // loss_scale
    row[10] = d.mask_terms ? d.mask_terms[2] : 0.f;                   // loss_iou
    row[11] = d.mask_terms ? d.mask_terms[4] : 0.f;                   // loss_error3d_align
#pragma unroll
    for (int i = 0; i < 12; ++i) d.row[i] = row[i];
    if (d.rows) {
#pragma unroll
      for (int i = 0; i < 12; ++i) d.rows[(size_t)d.row_index * 12 + i] = row[i];
    }
    if (d.meters) {                              // AverageValueMeter.add (:649-660): sum += value, n += 1
      double* sum = (double*)d.meters;
#pragma unroll
      for (int i = 0; i < 12; ++i) sum[i] += (double)row[i];
      int64_t* count = (int64_t*)(sum + 12);
      count[0] += 1;
    }
  }
}

}  // namespace hrp

using namespace hrp;

extern "C" int hrp_sim2real_monitor(const hrp_sim2real_monitor_desc* d, void* stream) {
  HRP_REQUIRE(d, "sim2real_monitor: null descriptor");
  HRP_REQUIRE(d->pose && d->rot && d->trans && d->root_uv && d->depth && d->xyz_fk, "sim2real_monitor: null prediction");
  HRP_REQUIRE(d->gt_pose && d->gt_root_rot && d->gt_root_trans && d->gt_root_uv && d->gt_kp3d && d->gt_kp2d && d->mask && d->K,
              "sim2real_monitor: null ground truth or intrinsics");
  HRP_REQUIRE(d->row, "sim2real_monitor: null row");
  HRP_REQUIRE(d->B > 0, "sim2real_monitor: B=%d", d->B);
  HRP_REQUIRE(d->J > 0 && d->J <= HRP_FK_MAX_KP, "sim2real_monitor: J=%d (at most %d key-points)", d->J, HRP_FK_MAX_KP);
  HRP_REQUIRE(d->P > 0 && d->P <= HRP_FK_MAX_JOINTS, "sim2real_monitor: P=%d (at most %d joints)", d->P, HRP_FK_MAX_JOINTS);
  HRP_REQUIRE(d->image_size > 0.f, "sim2real_monitor: image_size=%g", (double)d->image_size);
  HRP_REQUIRE(!d->meters || ((uintptr_t)d->meters % 8) == 0, "sim2real_monitor: meters is not 8-byte aligned");
  if (d->rows)
    HRP_REQUIRE(d->row_index >= 0 && d->row_index < d->capacity, "sim2real_monitor: row %d of a capacity of %d", d->row_index, d->capacity);
  hipLaunchKernelGGL(sim2real_monitor_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *d);
  return check_launch("sim2real_monitor");
}
