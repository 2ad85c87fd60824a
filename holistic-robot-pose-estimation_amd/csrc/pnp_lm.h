// The Levenberg-Marquardt pieces that the PnP kernels share (pnp.hip: one 64-lane workgroup per sample, lane = point; pnp_pooled.hip:
// one 256-thread workgroup per problem, points strided over the threads): the wave sum, the rotation as a jet in the angle-axis vector,
// the residual of one point with its Jacobian in (w, t), the 6 x 6 Cholesky solve and the normalisation of the returned rotation.
// Device code only; every function has internal linkage, so each translation unit compiles its own copy.
#pragma once
#include "hrp_common.h"

namespace hrp {
namespace {

constexpr int PNP_LM_MAX_IT = 200;

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return __shfl(v, 0, 64);
}

// ---- rotation as a second-order jet in the angle-axis vector w --------------------------------------------------------------
// R(w) = I + A(s) [w]x + B(s) (w w^T - s I),  s = |w|^2,  A = sin(theta)/theta,  B = (1 - cos(theta))/theta^2: the exact Rodrigues
// formula, smooth through theta = 0 (series below s = 1e-2).  J2 carries value, gradient (3) and Hessian (6: 00 01 02 11 12 22).
struct J2 {
  double v, g[3], h[6];
};
__device__ __forceinline__ int hix(int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
}
__device__ __forceinline__ J2 jconst(double c) {
  J2 r;
  r.v = c;
#pragma unroll
  for (int a = 0; a < 3; ++a) r.g[a] = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) r.h[a] = 0.0;
  return r;
}
__device__ __forceinline__ J2 jadd(const J2& x, const J2& y, double sy = 1.0) {
  J2 r;
  r.v = x.v + sy * y.v;
#pragma unroll
  for (int a = 0; a < 3; ++a) r.g[a] = x.g[a] + sy * y.g[a];
#pragma unroll
  for (int a = 0; a < 6; ++a) r.h[a] = x.h[a] + sy * y.h[a];
  return r;
}
__device__ __forceinline__ J2 jmul(const J2& x, const J2& y) {
  J2 r;
  r.v = x.v * y.v;
#pragma unroll
  for (int a = 0; a < 3; ++a) r.g[a] = x.g[a] * y.v + x.v * y.g[a];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) {
      const int k = hix(a, b);
      r.h[k] = x.h[k] * y.v + x.v * y.h[k] + x.g[a] * y.g[b] + x.g[b] * y.g[a];
    }
  return r;
}
// f(s) as a jet from f, f', f'' at s.v
__device__ __forceinline__ J2 jfun(const J2& s, double f, double f1, double f2) {
  J2 r;
  r.v = f;
#pragma unroll
  for (int a = 0; a < 3; ++a) r.g[a] = f1 * s.g[a];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) r.h[hix(a, b)] = f1 * s.h[hix(a, b)] + f2 * s.g[a] * s.g[b];
  return r;
}

__device__ void rodrigues_jet(const double w[3], J2 R[3][3]) {
  J2 wj[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    wj[a] = jconst(w[a]);
    wj[a].g[a] = 1.0;
  }
  const J2 s = jadd(jadd(jmul(wj[0], wj[0]), jmul(wj[1], wj[1])), jmul(wj[2], wj[2]));
  const double x = s.v;
  double A, A1, A2, B, B1, B2;
  if (x < 1e-2) {
    A = 1.0 + x * (-1.0 / 6 + x * (1.0 / 120 + x * (-1.0 / 5040 + x / 362880)));
    A1 = -1.0 / 6 + x * (1.0 / 60 + x * (-1.0 / 1680 + x / 90720));
    A2 = 1.0 / 60 + x * (-1.0 / 840 + x / 30240);
    B = 0.5 + x * (-1.0 / 24 + x * (1.0 / 720 + x * (-1.0 / 40320 + x / 3628800)));
    B1 = -1.0 / 24 + x * (1.0 / 360 + x * (-1.0 / 13440 + x / 907200));
    B2 = 1.0 / 360 + x * (-1.0 / 6720 + x / 302400);
  } else {
    const double th = sqrt(x), c = cos(th);
    A = sin(th) / th;
    A1 = (c - A) / (2.0 * x);
    A2 = (-0.5 * A - 3.0 * A1) / (2.0 * x);
    B = (1.0 - c) / x;
    B1 = (0.5 * A - B) / x;
    B2 = (0.5 * A1 - 2.0 * B1) / x;
  }
  const J2 Aj = jfun(s, A, A1, A2), Bj = jfun(s, B, B1, B2);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      J2 e = jmul(Bj, jmul(wj[r], wj[c]));
      if (r == c) e = jadd(jadd(e, jmul(Bj, s), -1.0), jconst(1.0));
      // [w]x: (0,1) = -w2, (0,2) = w1, (1,0) = w2, (1,2) = -w0, (2,0) = -w1, (2,1) = w0
      if (r != c) {
        const int k = 3 - r - c;
        const double sg = ((r == 0 && c == 2) || (r == 1 && c == 0) || (r == 2 && c == 1)) ? 1.0 : -1.0;
        e = jadd(e, jmul(Aj, wj[k]), sg);
      }
      R[r][c] = e;
    }
}

// Cholesky of a symmetric positive definite N x N system; false if a pivot is not positive.
template <int N>
__device__ bool chol_solve(double (&A)[N][N], double (&b)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double d = A[k][k];
#pragma unroll
    for (int m = 0; m < k; ++m) d -= A[k][m] * A[k][m];
    if (!(d > 0.0)) return false;
    d = sqrt(d);
    A[k][k] = d;
#pragma unroll
    for (int r = k + 1; r < N; ++r) {
      double v = A[r][k];
#pragma unroll
      for (int m = 0; m < k; ++m) v -= A[r][m] * A[k][m];
      A[r][k] = v / d;
    }
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
    double v = b[r];
#pragma unroll
    for (int m = 0; m < r; ++m) v -= A[r][m] * b[m];
    b[r] = v / A[r][r];
  }
#pragma unroll
  for (int r = N - 1; r >= 0; --r) {
    double v = b[r];
#pragma unroll
    for (int m = r + 1; m < N; ++m) v -= A[m][r] * b[m];
    b[r] = v / A[r][r];
  }
  return true;
}

__device__ __forceinline__ double sq3(double a, double b, double c) { return a * a + b * b + c * c; }

// ---- per-lane projection with its Jacobian in (w, t) --------------------------------------------------------------------------
struct Pose {
  double w[3], t[3];
};

// residual e = pi(K, R X + t) - x and de/d(w, t) (2 x 6); valid only where the lane holds a point
__device__ __forceinline__ void residual_jac(const J2 (&R)[3][3], const double (&t)[3], const double (&K)[9], const double (&X)[3],
                                             const double (&x)[2], double (&e)[2], double (&J)[2][6]) {
  double c[3], dc[6][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    c[r] = R[r][0].v * X[0] + R[r][1].v * X[1] + R[r][2].v * X[2] + t[r];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      dc[a][r] = R[r][0].g[a] * X[0] + R[r][1].g[a] * X[1] + R[r][2].g[a] * X[2];
      dc[3 + a][r] = r == a ? 1.0 : 0.0;
    }
  }
  double P[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) P[r] = K[3 * r] * c[0] + K[3 * r + 1] * c[1] + K[3 * r + 2] * c[2];
  const double iS = 1.0 / P[2];
  const double pi0 = P[0] * iS, pi1 = P[1] * iS;
  e[0] = pi0 - x[0];
  e[1] = pi1 - x[1];
#pragma unroll
  for (int l = 0; l < 6; ++l) {
    double dP[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) dP[r] = K[3 * r] * dc[l][0] + K[3 * r + 1] * dc[l][1] + K[3 * r + 2] * dc[l][2];
    J[0][l] = (dP[0] - pi0 * dP[2]) * iS;
    J[1][l] = (dP[1] - pi1 * dP[2]) * iS;
  }
}

// rotation normalised to |w| <= pi
__device__ __forceinline__ void normalise_rotation(Pose& y) {
  double th = sqrt(sq3(y.w[0], y.w[1], y.w[2]));
  if (th > M_PI) {
    double tn = fmod(th, 2.0 * M_PI);
    if (tn > M_PI) tn -= 2.0 * M_PI;
    const double f = tn / th;
#pragma unroll
    for (int k = 0; k < 3; ++k) y.w[k] *= f;
  }
}

}  // namespace
}  // namespace hrp
