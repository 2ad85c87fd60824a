// Back-propagatable PnP (reference lib/utils/BPnP.py): EPnP start + Levenberg-Marquardt refinement on the GPU, and the
// reference's implicit-function backward.  One 64-lane workgroup per sample, lane i holds point i (n <= 64); fp32 in and out,
// fp64 inside.  Every cross-lane sum is a fixed-order butterfly whose lane-0 result is broadcast, so the values every lane
// branches on are identical and two identical calls return identical bytes.  Small dense systems live either in registers
// (compile-time indices only) or in LDS (the Jacobi eigen-solves, whose pivots are data dependent).
// The robust forward (pnp_robust_kernel) puts a consensus over P3P hypotheses in front of the same LM: lane = hypothesis while it
// hypothesises and scores (pnp_minimal.h), lane = point again for the refits.  The LM pieces that pnp_pooled.hip uses too (the wave sum,
// the rotation jet, a point's residual and Jacobian, the Cholesky solve) are in pnp_lm.h.
#include "hrp_common.h"
#include "pnp_minimal.h"
#include "pnp_lm.h"

namespace hrp {
namespace {

// The rotation the reference's backward differentiates (kornia's torchgeometry angle_axis_to_rotation_matrix, BPnP.py:184,
// geometries.py:164-235): axis k = w / (theta + 1e-6), R = cos I + sin [k]x + (1 - cos) k k^T, and I + [w]x where theta^2 <= 1e-6.
// The backward uses it so that its J_fy is the reference's; the difference from the exact formula is ~1e-6 / theta relative in R,
// which the 6 x 6 inverse amplifies to ~2e-4 of the gradients at theta ~ 0.14.
__device__ void rotation_ref_jet(const double w[3], J2 R[3][3]) {
  J2 wj[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    wj[a] = jconst(w[a]);
    wj[a].g[a] = 1.0;
  }
  const J2 s = jadd(jadd(jmul(wj[0], wj[0]), jmul(wj[1], wj[1])), jmul(wj[2], wj[2]));
  if (s.v > 1e-6) {
    const double th = sqrt(s.v);
    const J2 tj = jfun(s, th, 0.5 / th, -0.25 / (s.v * th));
    const double d = th + 1e-6;
    const J2 inv = jfun(tj, 1.0 / d, -1.0 / (d * d), 2.0 / (d * d * d));
    const J2 c = jfun(tj, cos(th), -sin(th), -cos(th)), sn = jfun(tj, sin(th), cos(th), -sin(th));
    const J2 omc = jadd(jconst(1.0), c, -1.0);
    J2 k[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) k[a] = jmul(wj[a], inv);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        J2 e = jmul(omc, jmul(k[r], k[q]));
        if (r == q) e = jadd(e, c);
        else {
          const double sg = ((r == 0 && q == 2) || (r == 1 && q == 0) || (r == 2 && q == 1)) ? 1.0 : -1.0;
          e = jadd(e, jmul(sn, k[3 - r - q]), sg);
        }
        R[r][q] = e;
      }
  } else {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        J2 e = jconst(r == q ? 1.0 : 0.0);
        if (r != q) {
          const double sg = ((r == 0 && q == 2) || (r == 1 && q == 0) || (r == 2 && q == 1)) ? 1.0 : -1.0;
          e = jadd(e, wj[3 - r - q], sg);
        }
        R[r][q] = e;
      }
  }
}

// ---- small dense solves, compile-time sizes (registers) ---------------------------------------------------------------------
// least squares over the 6 rows of L restricted to the columns in cols (normal equations)
template <int N>
__device__ void lsq6(const double* L, const int (&cols)[N], const double* rho, double (&x)[N]) {
  double A[N][N];
#pragma unroll
  for (int a = 0; a < N; ++a) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += L[r * 10 + cols[a]] * rho[r];
    x[a] = s;
#pragma unroll
    for (int b = 0; b < N; ++b) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) t += L[r * 10 + cols[a]] * L[r * 10 + cols[b]];
      A[a][b] = t;
    }
  }
  if (!chol_solve<N>(A, x)) {
#pragma unroll
    for (int a = 0; a < N; ++a) x[a] = 0.0;
  }
}

// EPnP Gauss-Newton on the four betas (5 iterations, as OpenCV's epnp::gauss_newton)
__device__ void betas_gauss_newton(const double* L, const double* rho, double (&bt)[4]) {
  for (int it = 0; it < 5; ++it) {
    double J[6][4], e[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double* l = L + r * 10;
      J[r][0] = 2 * l[0] * bt[0] + l[1] * bt[1] + l[3] * bt[2] + l[6] * bt[3];
      J[r][1] = l[1] * bt[0] + 2 * l[2] * bt[1] + l[4] * bt[2] + l[7] * bt[3];
      J[r][2] = l[3] * bt[0] + l[4] * bt[1] + 2 * l[5] * bt[2] + l[8] * bt[3];
      J[r][3] = l[6] * bt[0] + l[7] * bt[1] + l[8] * bt[2] + 2 * l[9] * bt[3];
      e[r] = rho[r] - (l[0] * bt[0] * bt[0] + l[1] * bt[0] * bt[1] + l[2] * bt[1] * bt[1] + l[3] * bt[0] * bt[2] +
                       l[4] * bt[1] * bt[2] + l[5] * bt[2] * bt[2] + l[6] * bt[0] * bt[3] + l[7] * bt[1] * bt[3] +
                       l[8] * bt[2] * bt[3] + l[9] * bt[3] * bt[3]);
    }
    double A[4][4], x[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) s += J[r][a] * e[r];
      x[a] = s;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) t += J[r][a] * J[r][b];
        A[a][b] = t;
      }
    }
    if (!chol_solve<4>(A, x)) return;
#pragma unroll
    for (int a = 0; a < 4; ++a) bt[a] += x[a];
  }
}

// ---- cyclic Jacobi eigen-solve of a symmetric n x n matrix in LDS (n <= 12) ------------------------------------------------------
// A (row-major) ends diagonal, V holds the eigenvectors as columns.  Lane k < n updates row / column k of each rotation; every
// lane reads the same pivots, so the control flow is uniform.
__device__ void jacobi_lds(double* A, double* V, int n, int lane) {
  for (int e = lane; e < n * n; e += 64) V[e] = (e / n == e % n) ? 1.0 : 0.0;
  __syncthreads();
  for (int sweep = 0; sweep < 32; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int p = 0; p < n; ++p) {
      dia += A[p * n + p] * A[p * n + p];
      for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
    }
    if (!(off > 1e-30 * dia)) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double app = A[p * n + p], aqq = A[q * n + q];
        const double th = (aqq - app) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        __syncthreads();
        if (lane < n) {
          const int k = lane;
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
        __syncthreads();
        if (lane < n) {
          const int k = lane;
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = k == q ? 0.0 : c * apk - s * aqk;
          A[q * n + k] = k == p ? 0.0 : s * apk + c * aqk;
        }
        __syncthreads();
      }
  }
  __syncthreads();
}

// cost = sum |e|^2, JtJ (upper triangle, 21) and Jte (6) over the sample's points
__device__ void lm_eval(const Pose& y, const double (&K)[9], const double (&X)[3], const double (&x)[2], bool on, double& cost,
                        double (&JtJ)[6][6], double (&Jte)[6]) {
  J2 R[3][3];
  rodrigues_jet(y.w, R);
  double e[2], J[2][6];
  residual_jac(R, y.t, K, X, x, e, J);
  if (!on) {
    e[0] = e[1] = 0.0;
#pragma unroll
    for (int l = 0; l < 6; ++l) J[0][l] = J[1][l] = 0.0;
  }
  cost = wsum(e[0] * e[0] + e[1] * e[1]);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    Jte[a] = wsum(J[0][a] * e[0] + J[1][a] * e[1]);
#pragma unroll
    for (int b = a; b < 6; ++b) JtJ[a][b] = JtJ[b][a] = wsum(J[0][a] * J[0][b] + J[1][a] * J[1][b]);
  }
}

__device__ __forceinline__ void quat_to_R(const double (&q)[4], double (&R)[3][3]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0][0] = 1 - 2 * (y * y + z * z); R[0][1] = 2 * (x * y - w * z); R[0][2] = 2 * (x * z + w * y);
  R[1][0] = 2 * (x * y + w * z); R[1][1] = 1 - 2 * (x * x + z * z); R[1][2] = 2 * (y * z - w * x);
  R[2][0] = 2 * (x * z - w * y); R[2][1] = 2 * (y * z + w * x); R[2][2] = 1 - 2 * (x * x + y * y);
}

// EPnP (Lepetit, Moreno-Noguer, Fua 2009) as OpenCV's SOLVEPNP_EPNP: returns the best of the N = 1, 2, 3 beta solutions
__device__ __forceinline__ Pose epnp(const double (&K)[9], const double (&X)[3], const double (&x)[2], bool on, int n, int lane, double* sA, double* sV,
                     double* sN, double* sL, double* sRho) {
  const double m = on ? 1.0 : 0.0, inv_n = 1.0 / n;
  // control points: centroid + principal axes scaled by sqrt(eigenvalue / n)
  double cw[4][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) cw[0][k] = wsum(m * X[k]) * inv_n;
  const double d[3] = {m * (X[0] - cw[0][0]), m * (X[1] - cw[0][1]), m * (X[2] - cw[0][2])};
  double cov[6];
  cov[0] = wsum(d[0] * d[0]); cov[1] = wsum(d[0] * d[1]); cov[2] = wsum(d[0] * d[2]);
  cov[3] = wsum(d[1] * d[1]); cov[4] = wsum(d[1] * d[2]); cov[5] = wsum(d[2] * d[2]);
  if (lane == 0) {
    sA[0] = cov[0]; sA[1] = sA[3] = cov[1]; sA[2] = sA[6] = cov[2];
    sA[4] = cov[3]; sA[5] = sA[7] = cov[4]; sA[8] = cov[5];
  }
  __syncthreads();
  jacobi_lds(sA, sV, 3, lane);
  // eigenvalues in descending order
  int o0 = 0, o1 = 1, o2 = 2;
  {
    const double l0 = sA[0], l1 = sA[4], l2 = sA[8];
    if (l1 > l0 && l1 >= l2) { o0 = 1; o1 = 0; }
    else if (l2 > l0 && l2 > l1) { o0 = 2; o2 = 0; }
    const double la = sA[o1 * 4], lb = sA[o2 * 4];
    if (lb > la) { const int t = o1; o1 = o2; o2 = t; }
  }
  const int ord[3] = {o0, o1, o2};
  double u[3][3], kk[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    kk[j] = sqrt(fmax(sA[ord[j] * 4], 0.0) * inv_n);
#pragma unroll
    for (int r = 0; r < 3; ++r) u[j][r] = sV[r * 3 + ord[j]];
  }
  const double kmin = 1e-9 * fmax(kk[0], 1e-300);
  double alpha[4];
  alpha[0] = 1.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double kj = fmax(kk[j], kmin);
#pragma unroll
    for (int r = 0; r < 3; ++r) cw[j + 1][r] = cw[0][r] + kj * u[j][r];
    alpha[j + 1] = (u[j][0] * d[0] + u[j][1] * d[1] + u[j][2] * d[2]) / kj;
    alpha[0] -= alpha[j + 1];
  }
  // M^T M of the 2n x 12 system (OpenCV epnp::fill_M)
  const double fu = K[0], fv = K[4], uc = K[2], vc = K[5];
  double m1[12], m2[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double a = m * alpha[j];
    m1[3 * j] = a * fu; m1[3 * j + 1] = 0.0; m1[3 * j + 2] = a * (uc - x[0]);
    m2[3 * j] = 0.0; m2[3 * j + 1] = a * fv; m2[3 * j + 2] = a * (vc - x[1]);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 12; ++r)
#pragma unroll
    for (int c = r; c < 12; ++c) {
      const double v = wsum(m1[r] * m1[c] + m2[r] * m2[c]);
      if (lane == 0) sA[r * 12 + c] = sA[c * 12 + r] = v;
    }
  __syncthreads();
  jacobi_lds(sA, sV, 12, lane);
  // the four eigenvectors of the smallest eigenvalues into sN[i][12], ascending: i = 0 the smallest (OpenCV's ut + 12 * 11)
  {
    int used = 0, idx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int best = -1;
      double bv = 0.0;
      for (int k = 0; k < 12; ++k) {
        const double ev = sA[k * 13];
        if (!((used >> k) & 1) && (best < 0 || ev < bv)) { best = k; bv = ev; }
      }
      used |= 1 << best;
      idx[i] = best;
    }
    __syncthreads();
    if (lane < 48) sN[lane] = sV[(lane % 12) * 12 + (lane / 12 == 0 ? idx[0] : lane / 12 == 1 ? idx[1] : lane / 12 == 2 ? idx[2] : idx[3])];
    __syncthreads();
  }
  // L_6x10 and rho (OpenCV epnp::compute_L_6x10, compute_rho)
  if (lane == 0) {
    constexpr int PA[6] = {0, 0, 0, 1, 1, 2}, PB[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double dv[4][3];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) dv[i][k] = sN[i * 12 + 3 * PA[j] + k] - sN[i * 12 + 3 * PB[j] + k];
      auto dot = [&](int a, int b) { return dv[a][0] * dv[b][0] + dv[a][1] * dv[b][1] + dv[a][2] * dv[b][2]; };
      double* L = sL + j * 10;
      L[0] = dot(0, 0); L[1] = 2 * dot(0, 1); L[2] = dot(1, 1); L[3] = 2 * dot(0, 2); L[4] = 2 * dot(1, 2);
      L[5] = dot(2, 2); L[6] = 2 * dot(0, 3); L[7] = 2 * dot(1, 3); L[8] = 2 * dot(2, 3); L[9] = dot(3, 3);
      sRho[j] = sq3(cw[PA[j]][0] - cw[PB[j]][0], cw[PA[j]][1] - cw[PB[j]][1], cw[PA[j]][2] - cw[PB[j]][2]);
    }
  }
  __syncthreads();
  const double* L = sL;
  const double* rho = sRho;
  double betas[3][4];
  {  // N = 1 (epnp::find_betas_approx_1)
    const int cols[4] = {0, 1, 3, 6};
    double b4[4];
    lsq6<4>(L, cols, rho, b4);
    const double s = sqrt(fabs(b4[0])), sg = b4[0] < 0 ? -1.0 : 1.0, is = s > 0 ? 1.0 / s : 0.0;
    betas[0][0] = s; betas[0][1] = sg * b4[1] * is; betas[0][2] = sg * b4[2] * is; betas[0][3] = sg * b4[3] * is;
  }
  {  // N = 2 (find_betas_approx_2)
    const int cols[3] = {0, 1, 2};
    double b3[3];
    lsq6<3>(L, cols, rho, b3);
    double b0, b1;
    if (b3[0] < 0) { b0 = sqrt(-b3[0]); b1 = b3[2] < 0 ? sqrt(-b3[2]) : 0.0; }
    else { b0 = sqrt(b3[0]); b1 = b3[2] > 0 ? sqrt(b3[2]) : 0.0; }
    if (b3[1] < 0) b0 = -b0;
    betas[1][0] = b0; betas[1][1] = b1; betas[1][2] = 0.0; betas[1][3] = 0.0;
  }
  {  // N = 3 (find_betas_approx_3)
    const int cols[5] = {0, 1, 2, 3, 4};
    double b5[5];
    lsq6<5>(L, cols, rho, b5);
    double b0, b1;
    if (b5[0] < 0) { b0 = sqrt(-b5[0]); b1 = b5[2] < 0 ? sqrt(-b5[2]) : 0.0; }
    else { b0 = sqrt(b5[0]); b1 = b5[2] > 0 ? sqrt(b5[2]) : 0.0; }
    if (b5[1] < 0) b0 = -b0;
    betas[2][0] = b0; betas[2][1] = b1; betas[2][2] = b0 != 0.0 ? b5[3] / b0 : 0.0; betas[2][3] = 0.0;
  }
  Pose best;
  double best_err = 0.0;
#pragma unroll
  for (int N = 0; N < 3; ++N) {
    betas_gauss_newton(L, rho, betas[N]);
    // camera-frame control points and this lane's point (epnp::compute_ccs, compute_pcs, solve_for_sign)
    double ccs[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        ccs[j][k] = betas[N][0] * sN[3 * j + k] + betas[N][1] * sN[12 + 3 * j + k] + betas[N][2] * sN[24 + 3 * j + k] +
                    betas[N][3] * sN[36 + 3 * j + k];
    double pc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) pc[k] = alpha[0] * ccs[0][k] + alpha[1] * ccs[1][k] + alpha[2] * ccs[2][k] + alpha[3] * ccs[3][k];
    const double sgn = __shfl(pc[2], 0, 64) < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) pc[k] *= sgn;
    // absolute orientation world -> camera (Horn 1987: quaternion of the largest eigenvalue)
    double pc0[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) pc0[k] = wsum(m * pc[k]) * inv_n;
    const double cc[3] = {m * (pc[0] - pc0[0]), m * (pc[1] - pc0[1]), m * (pc[2] - pc0[2])};
    double S[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) S[a][b] = wsum(d[a] * cc[b]);
    __syncthreads();
    if (lane == 0) {
      const double Nm[16] = {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0],
                             S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2],
                             S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1],
                             S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]};
      for (int k = 0; k < 16; ++k) sA[k] = Nm[k];
    }
    __syncthreads();
    jacobi_lds(sA, sV, 4, lane);
    int top = 0;
    for (int k = 1; k < 4; ++k)
      if (sA[k * 5] > sA[top * 5]) top = k;
    double q[4];
    double qn = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k] = sV[k * 4 + top]; qn += q[k] * q[k]; }
    qn = 1.0 / sqrt(qn);
    if (q[0] < 0.0) qn = -qn;
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] *= qn;
    double R[3][3];
    quat_to_R(q, R);
    Pose P;
#pragma unroll
    for (int r = 0; r < 3; ++r) P.t[r] = pc0[r] - (R[r][0] * cw[0][0] + R[r][1] * cw[0][1] + R[r][2] * cw[0][2]);
    // angle-axis of q (w >= 0)
    const double vn = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double f = vn > 1e-300 ? 2.0 * atan2(vn, q[0]) / vn : 2.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) P.w[k] = f * q[k + 1];
    // mean reprojection distance (epnp::reprojection_error)
    double cam[3], p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + P.t[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = K[3 * r] * cam[0] + K[3 * r + 1] * cam[1] + K[3 * r + 2] * cam[2];
    const double du = p[0] / p[2] - x[0], dvv = p[1] / p[2] - x[1];
    const double err = wsum(on ? sqrt(du * du + dvv * dvv) : 0.0) * inv_n;
    if (N == 0 || err < best_err) { best = P; best_err = err; }
  }
  return best;
}

// Levenberg-Marquardt on (w, t) over the lanes with `on` set: the objective of SOLVEPNP_ITERATIVE, Marquardt's diagonal damping.
// y is refined in place; cost = the sum of squares at y, it = trials, converged = 1 unless the trial cap ended the loop.
__device__ __forceinline__ void lm_refine(Pose& y, const double (&K)[9], const double (&X)[3], const double (&x)[2], bool on, double& cost,
                         int& it, int& converged) {
  double JtJ[6][6], Jte[6];
  lm_eval(y, K, X, x, on, cost, JtJ, Jte);
  double lambda = 1e-3;
  it = 0;
  converged = 0;
  for (; it < PNP_LM_MAX_IT; ++it) {
    double A[6][6], st[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c = 0; c < 6; ++c) A[a][c] = JtJ[a][c];
      A[a][a] += lambda * JtJ[a][a];
      st[a] = -Jte[a];
    }
    if (chol_solve<6>(A, st)) {
      Pose yn;
      double smax = 0.0, ymax = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        yn.w[k] = y.w[k] + st[k];
        yn.t[k] = y.t[k] + st[3 + k];
        smax = fmax(smax, fmax(fabs(st[k]), fabs(st[3 + k])));
        ymax = fmax(ymax, fmax(fabs(y.w[k]), fabs(y.t[k])));
      }
      double cn, JtJn[6][6], Jten[6];
      lm_eval(yn, K, X, x, on, cn, JtJn, Jten);
      if (cn < cost) {
        y = yn;
        cost = cn;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          Jte[a] = Jten[a];
#pragma unroll
          for (int c = 0; c < 6; ++c) JtJ[a][c] = JtJn[a][c];
        }
        lambda = fmax(lambda * 0.1, 1e-12);
        if (smax <= 1e-12 * (1.0 + ymax)) { converged = 1; ++it; break; }
        continue;
      }
    }
    lambda *= 10.0;
    // no step of any length lowers the cost at this precision: the minimum is reached
    if (lambda > 1e10) { converged = 1; ++it; break; }
  }
}

__global__ __launch_bounds__(64) void pnp_solve_kernel(const float* __restrict__ pts2d, const float* __restrict__ pts3d, int z_stride,
                                                       const float* __restrict__ Km, int K_stride, const float* __restrict__ ini_pose,
                                                       int n, float* __restrict__ P6d, int* __restrict__ status, float* __restrict__ rms) {
  __shared__ double sA[144], sV[144], sN[48], sL[60], sRho[6];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool on = lane < n;
  const int li = on ? lane : 0;
  double K[9], X[3], x[2];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = Km[(size_t)b * K_stride + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = pts3d[(size_t)b * z_stride + li * 3 + k];
  x[0] = pts2d[((size_t)b * n + li) * 2];
  x[1] = pts2d[((size_t)b * n + li) * 2 + 1];

  Pose y;
  if (ini_pose) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      y.w[k] = ini_pose[b * 6 + k];
      y.t[k] = ini_pose[b * 6 + 3 + k];
    }
  } else {
    y = epnp(K, X, x, on, n, lane, sA, sV, sN, sL, sRho);
  }

  double cost;
  int it, converged;
  lm_refine(y, K, X, x, on, cost, it, converged);
  normalise_rotation(y);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      P6d[b * 6 + k] = (float)y.w[k];
      P6d[b * 6 + 3 + k] = (float)y.t[k];
    }
    if (status) {
      status[b * 2] = converged;
      status[b * 2 + 1] = it;
    }
    if (rms) rms[b] = (float)sqrt(cost / n);
  }
}

// ---- robust forward: consensus over P3P hypotheses, then LM on the consensus set (pnp_minimal.h holds the per-hypothesis core) -------
// The reference's BPnP_fast starts from cv2.solvePnPRansac (BPnP.py:267); here the minimal sets are enumerated, not drawn, and each is
// solved by P3P.  Lane = hypothesis in passes of 64 (each lane solves its triple and scores every root against the sample's usable
// points, which lie in LDS), a butterfly picks the winner by (count, -ssq, lower hypothesis), then lane = point again: LM on the
// winner's inliers, re-score, refit while the set changes (three refits at most), and with refine_all one more LM over all usable points.
// Below min_inliers the sample takes pnp_solve_kernel's path (EPnP + LM) over its usable points.
__device__ __forceinline__ bool lane_inlier(const Pose& y, const double (&K)[9], const double (&X)[3], const double (&x)[2], double thr2) {
  double R[3][3], e2;
  pnpmin::aa_to_rot(y.w, R);
  return pnpmin::reproj_e2(R, y.t, K, X, x, e2) && e2 < thr2;
}

__global__ __launch_bounds__(64) void pnp_robust_kernel(const float* __restrict__ pts2d, const float* __restrict__ pts3d, int z_stride,
                                                        const float* __restrict__ Km, int K_stride, const unsigned char* __restrict__ valid,
                                                        int n, double thr, int min_inliers, int max_hypotheses, unsigned seed, int refine_all,
                                                        float* __restrict__ P6d, unsigned char* __restrict__ inliers,
                                                        int* __restrict__ status, float* __restrict__ rms) {
  __shared__ double sA[144], sV[144], sN[48], sL[60], sRho[6];
  __shared__ double sX[64][3], sx[64][2], sF[64][3];
  __shared__ int sIdx[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const double thr2 = thr * thr;
  double K[9], X[3], x[2], F[3] = {0.0, 0.0, 1.0};
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = Km[(size_t)b * K_stride + k];
  bool ok = lane < n;
  {
    const int li = ok ? lane : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = pts3d[(size_t)b * z_stride + li * 3 + k];
    x[0] = pts2d[((size_t)b * n + li) * 2];
    x[1] = pts2d[((size_t)b * n + li) * 2 + 1];
    ok = ok && pnpmin::point_valid(valid ? valid + (size_t)b * n + li : nullptr, X, x) && pnpmin::bearing(K, x, F);
  }
  // the usable points, compacted in lane order; a lane without one holds a copy of the first (as pnp_solve_kernel's idle lanes hold
  // point 0), so that nothing non-finite enters the sums it is masked out of
  const unsigned long long vmask = __ballot(ok);
  const int m = __popcll(vmask);
  const int first = m ? __ffsll((long long)vmask) - 1 : 0;
  if (ok) sIdx[__popcll(vmask & ((1ull << lane) - 1ull))] = lane;
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = pts3d[(size_t)b * z_stride + first * 3 + k];
    x[0] = pts2d[((size_t)b * n + first) * 2];
    x[1] = pts2d[((size_t)b * n + first) * 2 + 1];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    sX[lane][k] = X[k];
    sF[lane][k] = F[k];
  }
  sx[lane][0] = x[0];
  sx[lane][1] = x[1];
  __syncthreads();

  // hypothesise and score
  const int H = pnpmin::hypothesis_count(m, max_hypotheses);
  int best_count = -1, best_h = 0x7fffffff;
  double best_ssq = 0.0, bR[3][3], bt[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    bt[r] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) bR[r][k] = r == k ? 1.0 : 0.0;
  }
  for (int h = lane; h < H; h += 64) {
    int tri[3];
    pnpmin::hypothesis_triple(h, m, max_hypotheses, seed, tri[0], tri[1], tri[2]);
    double X3[3][3], f3[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int p = sIdx[tri[a]];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        X3[a][k] = sX[p][k];
        f3[a][k] = sF[p][k];
      }
    }
    pnpmin::P3P S;
    pnpmin::p3p_prepare(X3, f3, S);
#pragma nounroll
    for (int slot = 0; slot < 4; ++slot) {
      double R[3][3], t[3];
      if (!pnpmin::p3p_pose(S, slot, R, t)) continue;
      int count = 0;
      double ssq = 0.0;
      for (int q = 0; q < m; ++q) {
        const int p = sIdx[q];
        const double Xp[3] = {sX[p][0], sX[p][1], sX[p][2]}, xp[2] = {sx[p][0], sx[p][1]};
        double e2;
        if (pnpmin::reproj_e2(R, t, K, Xp, xp, e2) && e2 < thr2) {
          ++count;
          ssq += e2;
        }
      }
      if (pnpmin::score_better(count, ssq, best_count, best_ssq)) {
        best_count = count;
        best_ssq = ssq;
        best_h = h;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          bt[r] = t[r];
#pragma unroll
          for (int k = 0; k < 3; ++k) bR[r][k] = R[r][k];
        }
      }
    }
  }
  // the winner: more inliers, then the smaller sum of squares, then the lower hypothesis (a lane's own ties went to the lower
  // hypothesis and root already); the order is total, so every lane ends with the same triple
  {
    int wc = best_count, wh = best_h;
    double ws = best_ssq;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int oc = __shfl_xor(wc, o, 64), oh = __shfl_xor(wh, o, 64);
      const double os = __shfl_xor(ws, o, 64);
      if (pnpmin::score_better(oc, os, wc, ws) || (oc == wc && os == ws && oh < wh)) {
        wc = oc;
        ws = os;
        wh = oh;
      }
    }
    const int src = wh & 63;
    best_count = wc;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      bt[r] = __shfl(bt[r], src, 64);
#pragma unroll
      for (int k = 0; k < 3; ++k) bR[r][k] = __shfl(bR[r][k], src, 64);
    }
  }
  const bool consensus = best_count >= min_inliers;      // the same in every lane

  Pose y;
  bool fit;
  if (consensus) {
    pnpmin::rot_to_aa(bR, y.w);
#pragma unroll
    for (int k = 0; k < 3; ++k) y.t[k] = bt[k];
    double e2;
    fit = ok && pnpmin::reproj_e2(bR, bt, K, X, x, e2) && e2 < thr2;
  } else {
    y = epnp(K, X, x, ok, m, lane, sA, sV, sN, sL, sRho);
    fit = ok;
  }
  double cost = 0.0;
  int its = 0, converged = 0, nfit = 0;
  bool over_all = false;
  for (int round = 0;; ++round) {
    int it;
    lm_refine(y, K, X, x, fit, cost, it, converged);
    its += it;
    const unsigned long long fmask = __ballot(fit);
    nfit = __popcll(fmask);
    if (!consensus || over_all) break;
    const bool in = ok && lane_inlier(y, K, X, x, thr2);
    if (__ballot(in) != fmask && round < 2) {
      fit = in;
      continue;
    }
    if (!refine_all) break;
    fit = ok;
    over_all = true;
  }
  normalise_rotation(y);
  const bool in = ok && lane_inlier(y, K, X, x, thr2);
  const int count = __popcll(__ballot(in));
  if (lane < n) inliers[(size_t)b * n + lane] = in ? 1 : 0;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      P6d[b * 6 + k] = (float)y.w[k];
      P6d[b * 6 + 3 + k] = (float)y.t[k];
    }
    status[b * 4] = (consensus ? 0 : HRP_PNP_NO_CONSENSUS) | (converged ? HRP_PNP_CONVERGED : 0) | (m < 4 ? HRP_PNP_FEW_POINTS : 0);
    status[b * 4 + 1] = its;
    status[b * 4 + 2] = count;
    status[b * 4 + 3] = H;
    rms[b] = nfit ? (float)sqrt(cost / nfit) : 0.0f;
  }
}

// ---- backward: the reference's implicit-function gradient (BPnP.py:50-111, 154-236, fast variant :280-341) ----------------------
// f_j = sum_i coef_ij . r_i,  r_i = x_i S_i - (K [R|t] [z_i; 1])_{0:2},  coef_ij = -2 d pi_i / d y_j;  the rows of J_fy (6 x 6) and
// J_fK (6 x 9) are reduced over the points, J_fx (6 x 2) and J_fz (6 x 3) stay per lane.  `fast` drops the coef derivatives.
// mask (optional, [B, n] bytes): a point whose byte is 0 adds nothing to the reduced rows and gets zero grad_x / grad_z.
__global__ __launch_bounds__(64) void pnp_bwd_kernel(const float* __restrict__ pts2d, const float* __restrict__ pts3d, int z_stride,
                                                     const float* __restrict__ Km, int K_stride, const float* __restrict__ P6d,
                                                     const float* __restrict__ gout, int n, int fast, float* __restrict__ grad_x,
                                                     float* __restrict__ grad_z, float* __restrict__ grad_K, int* __restrict__ status,
                                                     const unsigned char* __restrict__ mask) {
  __shared__ double sR[3][3][10];  // the rotation jet: value, gradient (3), Hessian (6)
  __shared__ double sJy[6][6], sJK[6][9];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool on = lane < n;
  const int li = on ? lane : 0;
  const bool use = on && (!mask || mask[(size_t)b * n + li]);
  const double m = use ? 1.0 : 0.0;
  double K[9], X[3], x[2], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = Km[(size_t)b * K_stride + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = pts3d[(size_t)b * z_stride + li * 3 + k];
  x[0] = pts2d[((size_t)b * n + li) * 2];
  x[1] = pts2d[((size_t)b * n + li) * 2 + 1];
  if (mask && !use) {      // whatever a masked-out point holds (NaN included) stays out of the sums it is multiplied out of
    X[0] = X[1] = X[2] = 0.0;
    x[0] = x[1] = 0.0;
  }
  {
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      w[k] = P6d[b * 6 + k];
      t[k] = P6d[b * 6 + 3 + k];
    }
    J2 R[3][3];
    rotation_ref_jet(w, R);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          sR[r][c][0] = R[r][c].v;
#pragma unroll
          for (int a = 0; a < 3; ++a) sR[r][c][1 + a] = R[r][c].g[a];
#pragma unroll
          for (int a = 0; a < 6; ++a) sR[r][c][4 + a] = R[r][c].h[a];
        }
    }
  }
  __syncthreads();
  // camera point, projection, residual
  double c[3], P[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = sR[r][0][0] * X[0] + sR[r][1][0] * X[1] + sR[r][2][0] * X[2] + t[r];
#pragma unroll
  for (int r = 0; r < 3; ++r) P[r] = K[3 * r] * c[0] + K[3 * r + 1] * c[1] + K[3 * r + 2] * c[2];
  const double S = P[2], iS = 1.0 / S;
  const double pi[2] = {P[0] * iS, P[1] * iS};
  const double rr[2] = {x[0] * S - P[0], x[1] * S - P[1]};
  // first derivatives of P in the 6 pose and 3 point directions (K directions are sparse: dP_r / dK_(r,q) = c_q)
  double dc[9][3], dP[9][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      dc[a][r] = sR[r][0][1 + a] * X[0] + sR[r][1][1 + a] * X[1] + sR[r][2][1 + a] * X[2];
      dc[3 + a][r] = r == a ? 1.0 : 0.0;
      dc[6 + a][r] = sR[r][a][0];
    }
  }
#pragma unroll
  for (int w = 0; w < 9; ++w)
#pragma unroll
    for (int r = 0; r < 3; ++r) dP[w][r] = K[3 * r] * dc[w][0] + K[3 * r + 1] * dc[w][1] + K[3 * r + 2] * dc[w][2];
  auto dpi = [&](int k, const double* d) { return (d[k] - pi[k] * d[2]) * iS; };
  auto dres = [&](int k, const double* d) { return x[k] * d[2] - d[k]; };

  double Jx[6][2], Jz[6][3];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double pij[2] = {dpi(0, dP[j]), dpi(1, dP[j])};
    const double coef[2] = {-2.0 * pij[0], -2.0 * pij[1]};
    // contribution of this point to row j of J_fy, J_fz, J_fK; the coef-derivative term -2 d2pi/dy_j dw . r
    auto second = [&](const double* d2P, const double* dPw, double dPw2) -> double {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double d2pi = (d2P[k] - pi[k] * d2P[2] - pij[k] * dPw2 - dpi(k, dPw) * dP[j][2]) * iS;
        s += -2.0 * d2pi * rr[k];
      }
      return s;
    };
    double fy[6], fz[3], fK[9];
#pragma unroll
    for (int w = 0; w < 9; ++w) {
      double f = coef[0] * dres(0, dP[w]) + coef[1] * dres(1, dP[w]);
      if (!fast) {
        // d2c / dy_j dw: nonzero only for j a rotation component and w a rotation or point direction
        double d2c[3] = {0.0, 0.0, 0.0};
        if (j < 3 && w < 3) {
          const int h = hix(j, w);
#pragma unroll
          for (int r = 0; r < 3; ++r) d2c[r] = sR[r][0][4 + h] * X[0] + sR[r][1][4 + h] * X[1] + sR[r][2][4 + h] * X[2];
        } else if (j < 3 && w >= 6) {
#pragma unroll
          for (int r = 0; r < 3; ++r) d2c[r] = sR[r][w - 6][1 + j];
        }
        double d2P[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) d2P[r] = K[3 * r] * d2c[0] + K[3 * r + 1] * d2c[1] + K[3 * r + 2] * d2c[2];
        f += second(d2P, dP[w], dP[w][2]);
      }
      if (w < 6) fy[w] = f;
      else fz[w - 6] = f;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        // direction K_(r,q): dP = e_r c_q,  d2P / dy_j dK_(r,q) = e_r dc_j[q]
        double dPw[3] = {0.0, 0.0, 0.0};
        dPw[r] = c[q];
        double f = coef[0] * dres(0, dPw) + coef[1] * dres(1, dPw);
        if (!fast) {
          double d2P[3] = {0.0, 0.0, 0.0};
          d2P[r] = dc[j][q];
          f += second(d2P, dPw, dPw[2]);
        }
        fK[3 * r + q] = f;
      }
#pragma unroll
    for (int k = 0; k < 2; ++k) Jx[j][k] = coef[k] * S;
#pragma unroll
    for (int k = 0; k < 3; ++k) Jz[j][k] = fz[k];
#pragma unroll
    for (int l = 0; l < 6; ++l) {
      const double v = wsum(m * fy[l]);
      if (lane == 0) sJy[j][l] = v;
    }
#pragma unroll
    for (int l = 0; l < 9; ++l) {
      const double v = wsum(m * fK[l]);
      if (lane == 0) sJK[j][l] = v;
    }
  }
  __syncthreads();
  // J_fy^T v = g by LU with partial pivoting (row swaps as selects: every index compile-time)
  double A[6][6], v[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    v[a] = gout[b * 6 + a];
#pragma unroll
    for (int c2 = 0; c2 < 6; ++c2) A[a][c2] = sJy[c2][a];
  }
  bool singular = false;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int p = k;
    double pv = fabs(A[k][k]);
#pragma unroll
    for (int r = k + 1; r < 6; ++r)
      if (fabs(A[r][k]) > pv) { pv = fabs(A[r][k]); p = r; }
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const bool sw = r == p;
#pragma unroll
      for (int c2 = 0; c2 < 6; ++c2) {
        const double a = A[k][c2], bb = A[r][c2];
        A[k][c2] = sw ? bb : a;
        A[r][c2] = sw ? a : bb;
      }
      const double a = v[k], bb = v[r];
      v[k] = sw ? bb : a;
      v[r] = sw ? a : bb;
    }
    if (!(pv > 0.0)) singular = true;
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const double f = A[r][k] / A[k][k];
#pragma unroll
      for (int c2 = k; c2 < 6; ++c2) A[r][c2] -= f * A[k][c2];
      v[r] -= f * v[k];
    }
  }
#pragma unroll
  for (int r = 5; r >= 0; --r) {
    double s = v[r];
#pragma unroll
    for (int c2 = r + 1; c2 < 6; ++c2) s -= A[r][c2] * v[c2];
    v[r] = s / A[r][r];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a)
    if (!isfinite(v[a])) singular = true;
  if (singular) {
#pragma unroll
    for (int a = 0; a < 6; ++a) v[a] = __builtin_nan("");
  }
  // grad = -v^T J
  if (on) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) s -= v[j] * Jx[j][k];
      grad_x[((size_t)b * n + lane) * 2 + k] = use ? (float)s : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) s -= v[j] * Jz[j][k];
      grad_z[((size_t)b * n + lane) * 3 + k] = use ? (float)s : 0.0f;
    }
  }
  if (lane < 9) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) s -= v[j] * sJK[j][lane];
    grad_K[b * 9 + lane] = (float)s;
  }
  if (status && lane == 0) status[b] = singular ? 1 : 0;
}

// sum over the batch in sample order: out[e] = sum_b part[b * E + e]
__global__ __launch_bounds__(64) void pnp_batch_sum_kernel(const float* __restrict__ part, int B, int E, float* __restrict__ out) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= E) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += part[(size_t)b * E + e];
  out[e] = (float)s;
}

}  // namespace
}  // namespace hrp

using namespace hrp;

extern "C" int hrp_pnp_solve(const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride, const float* ini_pose,
                             int B, int n, float* P6d, int* status, float* rms, void* stream) {
  HRP_REQUIRE(pts2d && pts3d && K && P6d && B > 0, "pnp_solve: bad args");
  HRP_REQUIRE(n >= 4 && n <= 64, "pnp_solve: %d points (4..64 supported)", n);
  HRP_REQUIRE(pts3d_stride == 0 || pts3d_stride == 3 * n, "pnp_solve: pts3d stride %d (0 or 3n)", pts3d_stride);
  HRP_REQUIRE(K_stride == 0 || K_stride == 9, "pnp_solve: K stride %d (0 or 9)", K_stride);
  hipLaunchKernelGGL(pnp_solve_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pts2d, pts3d, pts3d_stride, K, K_stride, ini_pose, n,
                     P6d, status, rms);
  return check_launch("pnp_solve");
}

namespace {
int pnp_bwd_launch(const char* what, const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride, const float* P6d,
                   const float* grad_out, int B, int n, int fast, float* grad_x, float* grad_z, float* grad_K, float* grad_z_sum,
                   float* grad_K_sum, int* status, const unsigned char* mask, void* stream) {
  HRP_REQUIRE(pts2d && pts3d && K && P6d && grad_out && grad_x && grad_z && grad_K && B > 0, "%s: bad args", what);
  HRP_REQUIRE(n >= 4 && n <= 64, "%s: %d points (4..64 supported)", what, n);
  HRP_REQUIRE(pts3d_stride == 0 || pts3d_stride == 3 * n, "%s: pts3d stride %d (0 or 3n)", what, pts3d_stride);
  HRP_REQUIRE(K_stride == 0 || K_stride == 9, "%s: K stride %d (0 or 9)", what, K_stride);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pnp_bwd_kernel, dim3(B), dim3(64), 0, s, pts2d, pts3d, pts3d_stride, K, K_stride, P6d, grad_out, n, fast, grad_x,
                     grad_z, grad_K, status, mask);
  if (grad_z_sum) hipLaunchKernelGGL(pnp_batch_sum_kernel, dim3(cdiv(3 * n, 64)), dim3(64), 0, s, grad_z, B, 3 * n, grad_z_sum);
  if (grad_K_sum) hipLaunchKernelGGL(pnp_batch_sum_kernel, dim3(1), dim3(64), 0, s, grad_K, B, 9, grad_K_sum);
  return check_launch(what);
}
}  // namespace

extern "C" int hrp_pnp_bwd(const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride, const float* P6d,
                           const float* grad_out, int B, int n, int fast, float* grad_x, float* grad_z, float* grad_K, float* grad_z_sum,
                           float* grad_K_sum, int* status, void* stream) {
  return pnp_bwd_launch("pnp_bwd", pts2d, pts3d, pts3d_stride, K, K_stride, P6d, grad_out, B, n, fast, grad_x, grad_z, grad_K, grad_z_sum,
                        grad_K_sum, status, nullptr, stream);
}

extern "C" int hrp_pnp_bwd_masked(const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride, const float* P6d,
                                  const float* grad_out, const unsigned char* mask, int B, int n, int fast, float* grad_x, float* grad_z,
                                  float* grad_K, float* grad_z_sum, float* grad_K_sum, int* status, void* stream) {
  HRP_REQUIRE(mask, "pnp_bwd_masked: bad args");
  return pnp_bwd_launch("pnp_bwd_masked", pts2d, pts3d, pts3d_stride, K, K_stride, P6d, grad_out, B, n, fast, grad_x, grad_z, grad_K,
                        grad_z_sum, grad_K_sum, status, mask, stream);
}

extern "C" int hrp_pnp_solve_robust(const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride,
                                    const unsigned char* valid, int B, int n, double reproj_error, int min_inliers, int max_hypotheses,
                                    unsigned seed, int refine_all, float* P6d, unsigned char* inliers, int* status, float* rms, void* stream) {
  HRP_REQUIRE(pts2d && pts3d && K && P6d && inliers && status && rms && B > 0, "pnp_solve_robust: bad args");
  HRP_REQUIRE(n >= 4 && n <= 64, "pnp_solve_robust: %d points (4..64 supported)", n);
  HRP_REQUIRE(pts3d_stride == 0 || pts3d_stride == 3 * n, "pnp_solve_robust: pts3d stride %d (0 or 3n)", pts3d_stride);
  HRP_REQUIRE(K_stride == 0 || K_stride == 9, "pnp_solve_robust: K stride %d (0 or 9)", K_stride);
  HRP_REQUIRE(reproj_error > 0.0 && reproj_error <= 1e150, "pnp_solve_robust: reprojection threshold %g px (positive, finite)", reproj_error);
  HRP_REQUIRE(min_inliers >= 4 && min_inliers <= 64, "pnp_solve_robust: min_inliers %d (4..64)", min_inliers);
  HRP_REQUIRE(max_hypotheses >= 1 && max_hypotheses <= (1 << 20), "pnp_solve_robust: max_hypotheses %d (1..2^20)", max_hypotheses);
  hipLaunchKernelGGL(pnp_robust_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pts2d, pts3d, pts3d_stride, K, K_stride, valid, n,
                     reproj_error, min_inliers, max_hypotheses, seed, refine_all, P6d, inliers, status, rms);
  return check_launch("pnp_solve_robust");
}
