// Robust PnP, the per-hypothesis core: a minimal (three-point) pose solver, the enumeration of the minimal sets, and the score of a
// pose against all points.  Plain inline functions in fp64, the same for the kernel of pnp.hip (hrp_pnp_solve_robust) and for a host
// compiler (tests/pnp_minimal_host_check.cpp): PNPM_HD is the only thing that differs.  Nothing is allocated, nothing recurses, and no
// array is indexed by a run-time value (the device keeps everything in registers).
//
// P3P: Grunert's formulation (J. A. Grunert 1841, as restated by Haralick, Lee, Ottenberg, Noelle, "Review and analysis of solutions
// of the three point perspective pose estimation problem", IJCV 13(3), 1994, section 2.1).  With a, b, c the sides of the world
// triangle opposite to P1, P2, P3, the cosines of the angles between the bearings, and the depths s2 = u s1, s3 = v s1:
//   u = N(v) / D(v),  N = (p - 1) v^2 - 2 p cos(beta) v + p + 1,  D = 2 (cos(gamma) - v cos(alpha)),  p = (a^2 - c^2) / b^2,
//   N^2 - 2 cos(gamma) N D + M D^2 = 0,  M = 1 - (c^2 / b^2) (1 + v^2 - 2 v cos(beta)):   a quartic in v.
// The quartic's coefficients are formed here by multiplying those polynomials out, its real roots come from Ferrari's resolvent cubic
// (polished by Newton steps on the quartic), and every root's depths (s1, s2, s3) take two Newton steps on the three law-of-cosines
// equations themselves, so that the returned pose maps the three points onto their bearings to rounding error.  The pose follows from
// the two triangles by their orthonormal frames.  A root with a non-positive depth, a vanishing D, a residual of the three equations
// above 1e-10 of the squared sides, or the value of an earlier root (a repeated root) is dropped; collinear or coincident points,
// coincident bearings and non-finite input return no pose at all.  Nothing returned is NaN.
//
// Enumeration: hypothesis h of C(m, 3) is the h-th triple i < j < k in lexicographic order (unranking); where C(m, 3) exceeds the
// caller's budget, three distinct indices from a counter-based hash of (seed, h) instead (splitmix64; no state, the same on both sides).
// Score: (inlier count, -sum of the inliers' squared residuals); a point is an inlier when its camera depth is positive and its
// reprojection error is below the threshold, which a NaN or an infinite error never is.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PNPM_HD __host__ __device__ __forceinline__
#else
#define PNPM_HD inline
#endif

namespace pnpmin {

PNPM_HD bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN and +-inf

// a point can be used: its flag (optional) is set and its five coordinates are finite
PNPM_HD bool point_valid(const unsigned char* flag, const double (&X)[3], const double (&x)[2]) {
  if (flag && !*flag) return false;
  return finite64(X[0]) && finite64(X[1]) && finite64(X[2]) && finite64(x[0]) && finite64(x[1]);
}

// ---- enumeration of the minimal sets -----------------------------------------------------------------------------------------------
PNPM_HD int ncomb3(int m) { return m < 3 ? 0 : m * (m - 1) * (m - 2) / 6; }     // m <= 64: 41664 at most

PNPM_HD void unrank_triple(int h, int m, int& i, int& j, int& k) {
  int rem = h;
  for (i = 0; i < m - 3; ++i) {
    const int c = (m - 1 - i) * (m - 2 - i) / 2;     // triples that start with i
    if (rem < c) break;
    rem -= c;
  }
  for (j = i + 1; j < m - 2; ++j) {
    const int c = m - 1 - j;                         // triples that start with i, j
    if (rem < c) break;
    rem -= c;
  }
  k = j + 1 + rem;
}

PNPM_HD uint64_t splitmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// three distinct indices of [0, m), m >= 3, ascending, from (seed, h) alone
PNPM_HD void sample_triple(uint32_t seed, uint32_t h, int m, int& i, int& j, int& k) {
  const uint64_t key = ((uint64_t)seed << 32) | h;
  const uint64_t g = 0x9E3779B97F4A7C15ull;
  int a = (int)(splitmix64(key * 3 * g + g) % (uint64_t)m);
  int b = (int)(splitmix64(key * 3 * g + 2 * g) % (uint64_t)(m - 1));
  int c = (int)(splitmix64(key * 3 * g + 3 * g) % (uint64_t)(m - 2));
  if (b >= a) ++b;                                   // b among the m - 1 indices other than a
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  if (c >= lo) ++c;                                  // c among the m - 2 indices other than a, b
  if (c >= hi) ++c;
  i = lo < c ? lo : c;
  k = hi > c ? hi : c;
  j = lo + hi + c - i - k;
}

// the number of hypotheses for m usable points under a budget, and hypothesis h's triple (ranks in [0, m))
PNPM_HD int hypothesis_count(int m, int max_hypotheses) {
  const int total = m < 4 ? 0 : ncomb3(m);
  return total < max_hypotheses ? total : max_hypotheses;
}
PNPM_HD void hypothesis_triple(int h, int m, int max_hypotheses, uint32_t seed, int& i, int& j, int& k) {
  if (ncomb3(m) <= max_hypotheses) unrank_triple(h, m, i, j, k);
  else sample_triple(seed, (uint32_t)h, m, i, j, k);
}

// The same for the pooled solver (pnp_pooled.hip), whose m reaches 16384: ncomb3 leaves int beyond m = 2344.  min(C(m, 3), cap) in 64
// bits without forming a product above cap: of m, m - 1, m - 2 one factor gives up its 2 and one its 3, then a b c > cap is asked
// as a b > cap / c.
PNPM_HD int64_t ncomb3_capped(int m, int64_t cap) {
  if (m < 3 || cap <= 0) return 0;
  int64_t a = m, b = m - 1, c = m - 2;
  if (a % 2 == 0) a /= 2; else b /= 2;
  if (a % 3 == 0) a /= 3; else if (b % 3 == 0) b /= 3; else c /= 3;
  const int64_t ab = a * b;                          // below 2^62 for every int m
  return ab > cap / c ? cap : ab * c;
}
PNPM_HD int pooled_hypothesis_count(int m, int max_hypotheses) { return m < 4 ? 0 : (int)ncomb3_capped(m, max_hypotheses); }
PNPM_HD void pooled_hypothesis_triple(int h, int m, int max_hypotheses, uint32_t seed, int& i, int& j, int& k) {
  if (ncomb3_capped(m, (int64_t)max_hypotheses + 1) <= max_hypotheses) unrank_triple(h, m, i, j, k);
  else sample_triple(seed, (uint32_t)h, m, i, j, k);
}

// ---- small algebra -------------------------------------------------------------------------------------------------------------------
PNPM_HD double dot3(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PNPM_HD void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// the bearing of pixel x: K f = (x, y, 1) by the adjugate; false if K is singular or the result is not finite
PNPM_HD bool bearing(const double (&K)[9], const double (&x)[2], double (&f)[3]) {
  const double c0 = K[4] * K[8] - K[5] * K[7], c1 = K[5] * K[6] - K[3] * K[8], c2 = K[3] * K[7] - K[4] * K[6];
  const double det = K[0] * c0 + K[1] * c1 + K[2] * c2;
  if (!(fabs(det) > 0.0)) return false;
  const double id = 1.0 / det, r[3] = {x[0], x[1], 1.0};
  f[0] = (c0 * r[0] + (K[2] * K[7] - K[1] * K[8]) * r[1] + (K[1] * K[5] - K[2] * K[4]) * r[2]) * id;
  f[1] = (c1 * r[0] + (K[0] * K[8] - K[2] * K[6]) * r[1] + (K[2] * K[3] - K[0] * K[5]) * r[2]) * id;
  f[2] = (c2 * r[0] + (K[1] * K[6] - K[0] * K[7]) * r[1] + (K[0] * K[4] - K[1] * K[3]) * r[2]) * id;
  return finite64(f[0]) && finite64(f[1]) && finite64(f[2]);
}

// real roots of y^2 + B y + C = 0 into r0 >= r1; a discriminant within rounding of zero counts as zero
PNPM_HD bool quadratic_roots(double B, double C, double& r0, double& r1) {
  double disc = B * B - 4.0 * C;
  if (disc < 0.0) {
    if (disc < -1e-12 * (B * B + 4.0 * fabs(C))) return false;
    disc = 0.0;
  }
  const double s = sqrt(disc);
  const double qv = -0.5 * (B + (B >= 0.0 ? s : -s));
  double a = qv, b = qv != 0.0 ? C / qv : 0.0;
  if (qv == 0.0) a = b = 0.0;
  r0 = a > b ? a : b;
  r1 = a > b ? b : a;
  return true;
}

PNPM_HD bool quartic_same(double a, double b) { return fabs(a - b) <= 1e-6 * (1.0 + fabs(a) + fabs(b)); }

// real roots of c4 x^4 + c3 x^3 + c2 x^2 + c1 x + c0 into four fixed slots; the returned mask has bit s set where r[s] holds a root.
// Ferrari: depress, take the largest real root m of the resolvent cubic, split into two quadratics (slots 0, 1 and 2, 3).
PNPM_HD int quartic_real_roots(const double (&c)[5], double& x0, double& x1, double& x2, double& x3) {
  x0 = x1 = x2 = x3 = 0.0;
  const double big = fmax(fmax(fabs(c[0]), fabs(c[1])), fmax(fmax(fabs(c[2]), fabs(c[3])), fabs(c[4])));
  if (!finite64(big) || !(fabs(c[4]) > 1e-13 * big)) return 0;
  const double a = c[3] / c[4], b = c[2] / c[4], cc = c[1] / c[4], d = c[0] / c[4];
  const double p = b - 0.375 * a * a, q = cc - 0.5 * a * b + 0.125 * a * a * a;
  const double r = d - 0.25 * a * cc + 0.0625 * a * a * b - (3.0 / 256.0) * a * a * a * a;
  // m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0: negative or zero at m = 0, so its largest real root is >= 0
  const double k2 = p, k1 = 0.25 * p * p - r, k0 = -0.125 * q * q;
  const double P = k1 - k2 * k2 / 3.0, Q = 2.0 * k2 * k2 * k2 / 27.0 - k2 * k1 / 3.0 + k0;
  const double disc = 0.25 * Q * Q + P * P * P / 27.0;
  double t;
  if (disc > 0.0) {
    const double s = sqrt(disc);
    t = cbrt(-0.5 * Q + s) + cbrt(-0.5 * Q - s);
  } else if (P < 0.0) {
    const double rho = sqrt(-P / 3.0);
    double cs = -0.5 * Q / (rho * rho * rho);
    cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
    t = 2.0 * rho * cos(acos(cs) / 3.0);
  } else {
    t = 0.0;
  }
  double m = t - k2 / 3.0;
  for (int it = 0; it < 2; ++it) {
    const double f = ((m + k2) * m + k1) * m + k0, df = (3.0 * m + 2.0 * k2) * m + k1;
    if (fabs(df) > 0.0 && finite64(f / df)) m -= f / df;
  }
  if (!finite64(m)) return 0;
  int mask = 0;
  double y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
  const double scale = fabs(p) + sqrt(fabs(r)) + 1e-300;
  if (!(m > 1e-14 * scale)) {
    // q = 0 to rounding: y^4 + p y^2 + r = 0
    double z0, z1;
    if (quadratic_roots(p, r, z0, z1)) {
      if (z0 >= 0.0) { y0 = sqrt(z0); y1 = -y0; mask |= 3; }
      if (z1 >= 0.0) { y2 = sqrt(z1); y3 = -y2; mask |= 12; }
    }
  } else {
    const double sq = sqrt(2.0 * m), e = q / (2.0 * sq);
    if (quadratic_roots(-sq, 0.5 * p + m + e, y0, y1)) mask |= 3;
    if (quadratic_roots(sq, 0.5 * p + m - e, y2, y3)) mask |= 12;
  }
  x0 = y0 - 0.25 * a; x1 = y1 - 0.25 * a; x2 = y2 - 0.25 * a; x3 = y3 - 0.25 * a;
  for (int s = 0; s < 4; ++s) {
    double x = s == 0 ? x0 : (s == 1 ? x1 : (s == 2 ? x2 : x3));
    for (int it = 0; it < 2; ++it) {
      const double f = (((x + a) * x + b) * x + cc) * x + d, df = ((4.0 * x + 3.0 * a) * x + 2.0 * b) * x + cc;
      if (fabs(df) > 0.0 && finite64(f / df)) x -= f / df;
    }
    if (!finite64(x)) mask &= ~(1 << s);
    if (s == 0) x0 = x; else if (s == 1) x1 = x; else if (s == 2) x2 = x; else x3 = x;
  }
  // a repeated root is reported once: the later of two slots within 1e-6 of each other leaves the mask
  if ((mask & 1) && quartic_same(x1, x0)) mask &= ~2;
  if ((mask & 1) && quartic_same(x2, x0)) mask &= ~4;
  if ((mask & 2) && quartic_same(x2, x1)) mask &= ~4;
  if ((mask & 1) && quartic_same(x3, x0)) mask &= ~8;
  if ((mask & 2) && quartic_same(x3, x1)) mask &= ~8;
  if ((mask & 4) && quartic_same(x3, x2)) mask &= ~8;
  return mask;
}

// ---- P3P ----------------------------------------------------------------------------------------------------------------------------
struct P3P {
  double X[3][3];          // the world points
  double f[3][3];          // unit bearings
  double a2, b2, c2;       // |P2 - P3|^2, |P1 - P3|^2, |P1 - P2|^2
  double ca, cb, cg;       // f2 . f3, f1 . f3, f1 . f2
  double n2, n1, n0, d1, d0;
  double v0, v1, v2, v3;   // the quartic's roots, by slot (scalars: a run-time slot selects among them by value, in registers)
  int mask;                // accepted slots
};

// set the problem up and find the quartic's roots: the slots of `mask` may hold poses
PNPM_HD void p3p_prepare(const double (&X)[3][3], const double (&fin)[3][3], P3P& S) {
  S.mask = 0;
  S.v0 = S.v1 = S.v2 = S.v3 = 0.0;
  bool good = true;                                                   // (no early exit inside the loops: they unroll to fixed indices)
  for (int i = 0; i < 3; ++i) {
    const double nn = dot3(fin[i], fin[i]);
    good = good && finite64(nn) && nn > 0.0;
    const double inv = 1.0 / sqrt(nn);
    for (int k = 0; k < 3; ++k) {
      S.f[i][k] = fin[i][k] * inv;
      S.X[i][k] = X[i][k];
      good = good && finite64(X[i][k]);
    }
  }
  if (!good) return;
  double e12[3], e13[3], e23[3], nrm[3];
  for (int k = 0; k < 3; ++k) {
    e12[k] = X[1][k] - X[0][k];
    e13[k] = X[2][k] - X[0][k];
    e23[k] = X[2][k] - X[1][k];
  }
  S.a2 = dot3(e23, e23); S.b2 = dot3(e13, e13); S.c2 = dot3(e12, e12);
  if (!finite64(S.a2 + S.b2 + S.c2) || !(S.a2 > 0.0) || !(S.b2 > 0.0) || !(S.c2 > 0.0)) return;
  cross3(e12, e13, nrm);
  if (!(dot3(nrm, nrm) > 1e-8 * S.b2 * S.c2)) return;                  // collinear within 1e-4 rad
  S.ca = dot3(S.f[1], S.f[2]); S.cb = dot3(S.f[0], S.f[2]); S.cg = dot3(S.f[0], S.f[1]);
  const double cmax = fmax(S.ca, fmax(S.cb, S.cg));
  if (!(cmax < 1.0 - 1e-14)) return;                                  // two bearings coincide
  const double p = (S.a2 - S.c2) / S.b2, q = S.c2 / S.b2;
  S.n2 = p - 1.0; S.n1 = -2.0 * p * S.cb; S.n0 = p + 1.0;
  S.d1 = -2.0 * S.ca; S.d0 = 2.0 * S.cg;
  const double m2 = -q, m1 = 2.0 * q * S.cb, m0 = 1.0 - q;
  // N^2 - 2 cos(gamma) N D + M D^2
  const double g2 = -2.0 * S.cg;
  const double dd2 = S.d1 * S.d1, dd1 = 2.0 * S.d1 * S.d0, dd0 = S.d0 * S.d0;
  double c[5];
  c[4] = S.n2 * S.n2 + m2 * dd2;
  c[3] = 2.0 * S.n2 * S.n1 + g2 * S.n2 * S.d1 + m2 * dd1 + m1 * dd2;
  c[2] = S.n1 * S.n1 + 2.0 * S.n2 * S.n0 + g2 * (S.n2 * S.d0 + S.n1 * S.d1) + m2 * dd0 + m1 * dd1 + m0 * dd2;
  c[1] = 2.0 * S.n1 * S.n0 + g2 * (S.n1 * S.d0 + S.n0 * S.d1) + m1 * dd0 + m0 * dd1;
  c[0] = S.n0 * S.n0 + g2 * S.n0 * S.d0 + m0 * dd0;
  S.mask = quartic_real_roots(c, S.v0, S.v1, S.v2, S.v3);
}

// the pose of slot `slot` (compile-time or run-time: no array is indexed by it): R X + t maps the points onto their bearings.
// false, and the slot leaves the mask, where the root gives no pose.
PNPM_HD bool p3p_pose(P3P& S, int slot, double (&R)[3][3], double (&t)[3]) {
  if (!((S.mask >> slot) & 1)) return false;
  S.mask &= ~(1 << slot);
  const double v = slot == 0 ? S.v0 : (slot == 1 ? S.v1 : (slot == 2 ? S.v2 : S.v3));
  const double D = S.d1 * v + S.d0;
  if (!(fabs(D) > 1e-12)) return false;
  const double u = ((S.n2 * v + S.n1) * v + S.n0) / D;
  const double den = 1.0 + v * v - 2.0 * v * S.cb;
  if (!(u > 0.0) || !(v > 0.0) || !(den > 0.0)) return false;
  double s0 = sqrt(S.b2 / den), s1 = u * s0, s2 = v * s0;
  // Newton on the three law-of-cosines equations
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
  for (int it = 0; it < 3; ++it) {
    g0 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * S.ca - S.a2;
    g1 = s0 * s0 + s2 * s2 - 2.0 * s0 * s2 * S.cb - S.b2;
    g2 = s0 * s0 + s1 * s1 - 2.0 * s0 * s1 * S.cg - S.c2;
    if (it == 2) break;
    const double J01 = 2.0 * (s1 - s2 * S.ca), J02 = 2.0 * (s2 - s1 * S.ca);
    const double J10 = 2.0 * (s0 - s2 * S.cb), J12 = 2.0 * (s2 - s0 * S.cb);
    const double J20 = 2.0 * (s0 - s1 * S.cg), J21 = 2.0 * (s1 - s0 * S.cg);
    // J = [0 J01 J02; J10 0 J12; J20 J21 0]
    const double det = J01 * J12 * J20 + J02 * J10 * J21;
    const double jn = (fabs(J01) + fabs(J02)) * (fabs(J10) + fabs(J12)) * (fabs(J20) + fabs(J21));
    if (!(fabs(det) > 1e-9 * jn)) break;                              // a repeated root: the Jacobian is singular there
    const double id = 1.0 / det;
    const double m12 = J10 * g2 - g1 * J20;                           // Cramer's rule, the zero diagonal written out
    const double h0 = (-g0 * J12 * J21 + J01 * J12 * g2 + J02 * J21 * g1) * id;
    const double h1 = (g0 * J12 * J20 + J02 * m12) * id;
    const double h2 = (g0 * J10 * J21 - J01 * m12) * id;
    const double t0 = s0 - h0, t1 = s1 - h1, t2 = s2 - h2;
    if (!finite64(t0) || !finite64(t1) || !finite64(t2)) break;
    s0 = t0; s1 = t1; s2 = t2;
  }
  if (!(s0 > 0.0) || !(s1 > 0.0) || !(s2 > 0.0)) return false;
  const double tol = 1e-10 * (S.a2 + S.b2 + S.c2);
  if (!(fabs(g0) <= tol && fabs(g1) <= tol && fabs(g2) <= tol)) return false;
  // frames of the two triangles
  double Q[3][3], a1[3], a2v[3], wn[3], w1[3], w2[3], w3[3], c1[3], c2[3], c3[3];
  for (int k = 0; k < 3; ++k) {
    Q[0][k] = s0 * S.f[0][k]; Q[1][k] = s1 * S.f[1][k]; Q[2][k] = s2 * S.f[2][k];
  }
  for (int k = 0; k < 3; ++k) { a1[k] = S.X[1][k] - S.X[0][k]; a2v[k] = S.X[2][k] - S.X[0][k]; }
  double l = 1.0 / sqrt(dot3(a1, a1));
  for (int k = 0; k < 3; ++k) w1[k] = a1[k] * l;
  cross3(w1, a2v, wn);
  l = 1.0 / sqrt(dot3(wn, wn));
  for (int k = 0; k < 3; ++k) w3[k] = wn[k] * l;
  cross3(w3, w1, w2);
  for (int k = 0; k < 3; ++k) { a1[k] = Q[1][k] - Q[0][k]; a2v[k] = Q[2][k] - Q[0][k]; }
  const double q1 = dot3(a1, a1);
  if (!(q1 > 0.0)) return false;
  l = 1.0 / sqrt(q1);
  for (int k = 0; k < 3; ++k) c1[k] = a1[k] * l;
  cross3(c1, a2v, wn);
  const double q3 = dot3(wn, wn);
  if (!(q3 > 0.0)) return false;
  l = 1.0 / sqrt(q3);
  for (int k = 0; k < 3; ++k) c3[k] = wn[k] * l;
  cross3(c3, c1, c2);
  bool fin = true;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) {
      R[r][k] = c1[r] * w1[k] + c2[r] * w2[k] + c3[r] * w3[k];
      fin = fin && finite64(R[r][k]);
    }
  }
  for (int r = 0; r < 3; ++r) {
    t[r] = Q[0][r] - (R[r][0] * S.X[0][0] + R[r][1] * S.X[0][1] + R[r][2] * S.X[0][2]);
    fin = fin && finite64(t[r]);
  }
  if (!fin) return false;
  return true;
}

// all poses of a triple, in slot order: up to four (R, t); returns their number
PNPM_HD int p3p_solve(const double (&X)[3][3], const double (&f)[3][3], double (&R)[4][3][3], double (&t)[4][3]) {
  P3P S;
  p3p_prepare(X, f, S);
  int cnt = 0;
  for (int slot = 0; slot < 4; ++slot) {
    double Rs[3][3], ts[3];
    if (!p3p_pose(S, slot, Rs, ts)) continue;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) R[cnt][r][k] = Rs[r][k];
      t[cnt][r] = ts[r];
    }
    ++cnt;
  }
  return cnt;
}

// ---- rotation <-> angle-axis (exact Rodrigues; the quaternion by its largest component) ------------------------------------------------
PNPM_HD void aa_to_rot(const double (&w)[3], double (&R)[3][3]) {
  const double s = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double A, B;
  if (s < 1e-8) {
    A = 1.0 - s / 6.0;
    B = 0.5 - s / 24.0;
  } else {
    const double th = sqrt(s);
    A = sin(th) / th;
    B = (1.0 - cos(th)) / s;
  }
  R[0][0] = 1.0 - B * (w[1] * w[1] + w[2] * w[2]); R[0][1] = B * w[0] * w[1] - A * w[2]; R[0][2] = B * w[0] * w[2] + A * w[1];
  R[1][0] = B * w[0] * w[1] + A * w[2]; R[1][1] = 1.0 - B * (w[0] * w[0] + w[2] * w[2]); R[1][2] = B * w[1] * w[2] - A * w[0];
  R[2][0] = B * w[0] * w[2] - A * w[1]; R[2][1] = B * w[1] * w[2] + A * w[0]; R[2][2] = 1.0 - B * (w[0] * w[0] + w[1] * w[1]);
}

PNPM_HD void rot_to_aa(const double (&R)[3][3], double (&w)[3]) {
  double q0, q1, q2, q3;
  const double tr = R[0][0] + R[1][1] + R[2][2];
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(1.0 + tr);
    q0 = 0.25 * s; q1 = (R[2][1] - R[1][2]) / s; q2 = (R[0][2] - R[2][0]) / s; q3 = (R[1][0] - R[0][1]) / s;
  } else if (R[0][0] >= R[1][1] && R[0][0] >= R[2][2]) {
    const double s = 2.0 * sqrt(fmax(1.0 + R[0][0] - R[1][1] - R[2][2], 1e-300));
    q0 = (R[2][1] - R[1][2]) / s; q1 = 0.25 * s; q2 = (R[0][1] + R[1][0]) / s; q3 = (R[0][2] + R[2][0]) / s;
  } else if (R[1][1] >= R[2][2]) {
    const double s = 2.0 * sqrt(fmax(1.0 + R[1][1] - R[0][0] - R[2][2], 1e-300));
    q0 = (R[0][2] - R[2][0]) / s; q1 = (R[0][1] + R[1][0]) / s; q2 = 0.25 * s; q3 = (R[1][2] + R[2][1]) / s;
  } else {
    const double s = 2.0 * sqrt(fmax(1.0 + R[2][2] - R[0][0] - R[1][1], 1e-300));
    q0 = (R[1][0] - R[0][1]) / s; q1 = (R[0][2] + R[2][0]) / s; q2 = (R[1][2] + R[2][1]) / s; q3 = 0.25 * s;
  }
  if (q0 < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
  const double vn = sqrt(q1 * q1 + q2 * q2 + q3 * q3);
  const double f = vn > 1e-300 ? 2.0 * atan2(vn, q0) / vn : 2.0;
  w[0] = f * q1; w[1] = f * q2; w[2] = f * q3;
}

// ---- score -------------------------------------------------------------------------------------------------------------------------------
// squared reprojection error of X under (R, t) through K; false where the point lies behind the camera.  A caller compares e2 with
// its threshold by `e2 < thr2`, which is false for NaN and +inf.
PNPM_HD bool reproj_e2(const double (&R)[3][3], const double (&t)[3], const double (&K)[9], const double (&X)[3], const double (&x)[2],
                       double& e2) {
  double c[3], P[3];
  for (int r = 0; r < 3; ++r) c[r] = R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r];
  for (int r = 0; r < 3; ++r) P[r] = K[3 * r] * c[0] + K[3 * r + 1] * c[1] + K[3 * r + 2] * c[2];
  const double iS = 1.0 / P[2];
  const double du = P[0] * iS - x[0], dv = P[1] * iS - x[1];
  e2 = du * du + dv * dv;
  return c[2] > 0.0;
}

// (count, ssq) beats (bcount, bssq): more inliers, then the smaller sum of squares; equal scores keep the earlier candidate
PNPM_HD bool score_better(int count, double ssq, int bcount, double bssq) { return count > bcount || (count == bcount && ssq < bssq); }

}  // namespace pnpmin
