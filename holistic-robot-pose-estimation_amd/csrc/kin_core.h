// The kinematic refit (hrp_kin_solve, include/hrp.h): Levenberg-Marquardt on the free joint angles and, optionally, the camera pose of
// one sample, over the 2-D key-points, optional 3-D targets and a prior on the joints.  Everything but the launch lives here, written once
// for the kernel of kin.hip (one 64-lane workgroup per sample) and for a host compiler (tests/kinfit_host_check.cpp): KIN_HD and the `Par`
// policy are all that differ.  Par gives the lanes this caller executes, [lo(), hi()), and the barrier between two phases: the kernel runs
// lane threadIdx.x and __syncthreads(), the host check runs lanes 0..63 one after another and needs no barrier.  So every value that
// crosses a phase lies in KinShared (LDS on the device), every decision is taken from shared values, identically in each lane, and every
// sum runs in index order: two calls return the same bytes.
//
//   p = (free joints ascending, then w, t when the pose is free), fp64
//   value phase      lane = joint: its local pose, then its base-frame pose (the product along its ancestors, read from LDS);
//                    lane = key-point: X_k(p), its projection, the weighted residual rows
//   Jacobian phase   lane = parameter: its column in closed form from the frames and points the value phase left in LDS - for a revolute
//                    joint axis x (X_k - origin) on the key-points below it, for w the derivative of R(w) (a dual number through rot_aa).
//                    (A forward-mode dual carried through the whole FK, one lane per parameter, was written first: it needs no scratch
//                    either, but every lane then walks every key-point's chain with a sin / cos pair per joint, 37 us per LM trial on
//                    the Panda against 6 with the columns in closed form)
//   normal equations lane = row a of J^T J (a dot product per entry over the residual rows in index order), priors added analytically
//   Cholesky         right-looking in LDS, lane = matrix row, runtime size
// The FK arithmetic is that of heads.hip's templates (T = T_parent * origin * Rot(axis, q), camera_from_base's re-rooting), in fp64 on
// the chain's fp32 tables.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/hrp.h"

#if defined(__HIPCC__)
#define KIN_HD __host__ __device__ inline
#else
#define KIN_HD inline
#endif

namespace hrp {
namespace kin {

constexpr int KIN_LM_MAX_IT = HRP_KIN_MAX_IT;      // = PNP_LM_MAX_IT (pnp_lm.h): the schedule is lm_refine's
constexpr int KIN_MAX_PAR = HRP_FK_MAX_JOINTS + 6;
constexpr int KIN_LANES = 64;

KIN_HD bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and +-inf

// ---- scalars: double, or a double with one tangent ------------------------------------------------------------------------------------
struct DD {
  double v, d;
};
KIN_HD DD operator+(DD a, DD b) { return {a.v + b.v, a.d + b.d}; }
KIN_HD DD operator-(DD a, DD b) { return {a.v - b.v, a.d - b.d}; }
KIN_HD DD operator*(DD a, DD b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
KIN_HD DD operator/(DD a, DD b) {
  const double q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
template <class S> KIN_HD S lift(double v);
template <> KIN_HD double lift<double>(double v) { return v; }
template <> KIN_HD DD lift<DD>(double v) { return {v, 0.0}; }
KIN_HD double val(double a) { return a; }
KIN_HD double val(DD a) { return a.v; }
// f(s) from f and f' at s
KIN_HD double fun(double, double f, double) { return f; }
KIN_HD DD fun(DD s, double f, double f1) { return {f, f1 * s.d}; }

template <class S>
struct Rigid {      // 3x4 [R | t]
  S r[3][3], t[3];
};

template <class S>
KIN_HD Rigid<S> rigid_identity() {
  Rigid<S> T;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T.r[i][j] = lift<S>(i == j ? 1.0 : 0.0);
    T.t[i] = lift<S>(0.0);
  }
  return T;
}

template <class S>
KIN_HD Rigid<S> rigid_mul(const Rigid<S>& A, const Rigid<S>& B) {
  Rigid<S> C;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) C.r[i][j] = A.r[i][0] * B.r[0][j] + A.r[i][1] * B.r[1][j] + A.r[i][2] * B.r[2][j];
    C.t[i] = A.r[i][0] * B.t[0] + A.r[i][1] * B.t[1] + A.r[i][2] * B.t[2] + A.t[i];
  }
  return C;
}

// child pose of joint j relative to its parent, origin * motion(q), as 12 doubles (rows of [R | t]).  A joint whose column lies
// outside q is fixed.
KIN_HD Rigid<double> joint_local(const hrp_fk_chain* ch, int j, const double* q, int dof) {
  Rigid<double> O;
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) O.r[i][k] = (double)ch->origin[j][i * 4 + k];
    O.t[i] = (double)ch->origin[j][i * 4 + 3];
  }
  const int type = ch->type[j], cfg = ch->cfg[j];
  if (type == 0 || cfg < 0 || cfg >= dof) return O;
  const double qv = (double)ch->mimic_mul[j] * q[cfg] + (double)ch->mimic_off[j];
  const double a0 = (double)ch->axis[j][0], a1 = (double)ch->axis[j][1], a2 = (double)ch->axis[j][2];
  Rigid<double> M = rigid_identity<double>();
  if (type == 1) {
    const double s = sin(qv), c = cos(qv), omc = 1.0 - c;
    M.r[0][0] = c + omc * (a0 * a0); M.r[0][1] = omc * (a0 * a1) - s * a2; M.r[0][2] = omc * (a0 * a2) + s * a1;
    M.r[1][0] = omc * (a1 * a0) + s * a2; M.r[1][1] = c + omc * (a1 * a1); M.r[1][2] = omc * (a1 * a2) - s * a0;
    M.r[2][0] = omc * (a2 * a0) - s * a1; M.r[2][1] = omc * (a2 * a1) + s * a0; M.r[2][2] = c + omc * (a2 * a2);
  } else {
    M.t[0] = qv * a0; M.t[1] = qv * a1; M.t[2] = qv * a2;
  }
  return rigid_mul(O, M);
}
KIN_HD void store12(double* p, const Rigid<double>& T) {
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) p[4 * i + k] = T.r[i][k];
    p[4 * i + 3] = T.t[i];
  }
}
KIN_HD Rigid<double> load12(const double* p) {
  Rigid<double> T;
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) T.r[i][k] = p[4 * i + k];
    T.t[i] = p[4 * i + 3];
  }
  return T;
}
KIN_HD int chain_joints(const hrp_fk_chain* ch) {
  const int nj = ch->njoints;
  return nj < 0 ? 0 : (nj < HRP_FK_MAX_JOINTS ? nj : HRP_FK_MAX_JOINTS);
}
// the joints on the way from the base to the child frame of joint `leaf`, itself included, as a bit mask (leaf < 0: none).  A table
// that is no tree (a parent at or above its child, an index outside the chain) ends the walk instead of running on.
KIN_HD uint32_t ancestors(const hrp_fk_chain* ch, int leaf) {
  const int nj = chain_joints(ch);
  uint32_t mask = 0;
  for (int j = leaf; j >= 0 && j < nj && !(mask >> j & 1u);) {
    mask |= 1u << j;
    const int up = ch->parent[j];
    j = up < j ? up : -1;
  }
  return mask;
}

// R(w) = I + A(s) [w]x + B(s) (w w^T - s I), s = |w|^2: pnp_lm.h's rodrigues_jet to first order, smooth through 0
template <class S>
KIN_HD void rot_aa(const S (&w)[3], S (&R)[3][3]) {
  const S s = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double x = val(s);
  double A, A1, B, B1;
  if (x < 1e-2) {
    A = 1.0 + x * (-1.0 / 6 + x * (1.0 / 120 + x * (-1.0 / 5040 + x / 362880)));
    A1 = -1.0 / 6 + x * (1.0 / 60 + x * (-1.0 / 1680 + x / 90720));
    B = 0.5 + x * (-1.0 / 24 + x * (1.0 / 720 + x * (-1.0 / 40320 + x / 3628800)));
    B1 = -1.0 / 24 + x * (1.0 / 360 + x * (-1.0 / 13440 + x / 907200));
  } else {
    const double th = sqrt(x), c = cos(th);
    A = sin(th) / th;
    A1 = (c - A) / (2.0 * x);
    B = (1.0 - c) / x;
    B1 = (0.5 * A - B) / x;
  }
  const S Aj = fun(s, A, A1), Bj = fun(s, B, B1);
  // entry by entry, so that w is never indexed by a variable (an array indexed that way would live in scratch memory)
  const S one = lift<S>(1.0), Bs = Bj * s;
  const S a0 = Aj * w[0], a1 = Aj * w[1], a2 = Aj * w[2];
  const S b01 = Bj * (w[0] * w[1]), b02 = Bj * (w[0] * w[2]), b12 = Bj * (w[1] * w[2]);
  R[0][0] = Bj * (w[0] * w[0]) - Bs + one; R[0][1] = b01 - a2; R[0][2] = b02 + a1;
  R[1][0] = b01 + a2; R[1][1] = Bj * (w[1] * w[1]) - Bs + one; R[1][2] = b12 - a0;
  R[2][0] = b02 - a1; R[2][1] = b12 + a0; R[2][2] = Bj * (w[2] * w[2]) - Bs + one;
}

// base_to_cam's formula for six numbers (heads.hip; geometries.py:100-115): rows x, y, z from a = r6[0..2], b = r6[3..5]
KIN_HD void rot_from_6d(const double (&r6)[6], double (&R)[3][3]) {
  const double n = sqrt(r6[0] * r6[0] + r6[1] * r6[1] + r6[2] * r6[2]);
  const double x[3] = {r6[0] / n, r6[1] / n, r6[2] / n};
  double z[3] = {x[1] * r6[5] - x[2] * r6[4], x[2] * r6[3] - x[0] * r6[5], x[0] * r6[4] - x[1] * r6[3]};
  const double zn = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  for (int k = 0; k < 3; ++k) z[k] /= zn;
  const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
  for (int k = 0; k < 3; ++k) {
    R[0][k] = x[k];
    R[1][k] = y[k];
    R[2][k] = z[k];
  }
}

// angle-axis of a rotation matrix through its quaternion (pnp_minimal.h's rot_to_aa), |w| <= pi
KIN_HD void rot_to_aa(const double (&R)[3][3], double (&w)[3]) {
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

// uv = (K X)[:2] / (K X)[2] (transforms.py:17-21)
template <class S>
KIN_HD void project(const double* K, const S (&X)[3], S (&uv)[2]) {
  S h[3];
  for (int r = 0; r < 3; ++r) h[r] = lift<S>(K[3 * r]) * X[0] + lift<S>(K[3 * r + 1]) * X[1] + lift<S>(K[3 * r + 2]) * X[2];
  uv[0] = h[0] / h[2];
  uv[1] = h[1] / h[2];
}

// ---- one sample ---------------------------------------------------------------------------------------------------------------------------
struct Problem {      // this sample's pointers (NULL where the descriptor's is) and the launch's scalars
  const hrp_fk_chain* ch;
  const float *pts2d, *w2d, *pts3d, *w3d, *K, *q0, *rot0, *trans0, *q_lo, *q_hi, *prior_q;
  int nkp, dof, rot_dim, free_pose, root;
  uint32_t free_q;
  float *q, *rot, *trans, *xyz, *uv, *rms, *cov;
  int32_t* status;
};

KIN_HD int popcount32(uint32_t v) {
  int n = 0;
  for (; v; v &= v - 1) ++n;
  return n;
}
KIN_HD uint32_t free_mask(uint32_t free_q, int dof) { return dof >= 32 ? free_q : free_q & ((1u << dof) - 1u); }
KIN_HD int kin_npar(uint32_t free_q, int dof, int free_pose) { return popcount32(free_mask(free_q, dof)) + (free_pose ? 6 : 0); }
KIN_HD int kin_nrow(int nkp, int has3d) { return nkp * (has3d ? 5 : 2); }

// The sample's shared arrays, carved from one buffer of shared_doubles() doubles.  Only the base and the sizes are kept; every array
// is an offset computed where it is used (a pointer per array would cost the kernel 40 scalar registers).
struct Shared {
  double* base;
  int npar, nrow, nkp;
  KIN_HD size_t jsize() const {      // J [npar][nrow]; the covariance's inverse [npar][npar] and an evaluation's local joint poses reuse it
    const size_t a = (size_t)npar * (nrow > npar ? nrow : npar), b = 12 * HRP_FK_MAX_JOINTS;
    return a > b ? a : b;
  }
  KIN_HD double* J() const { return base; }                       // [npar][nrow] columns of the Jacobian
  KIN_HD double* M() const { return J() + jsize(); }              // [npar][npar] J^T J
  KIN_HD double* L() const { return M() + (size_t)npar * npar; }  // packed lower triangle
  KIN_HD double* Ld() const { return L() + (size_t)npar * (npar + 1) / 2; }
  KIN_HD double* g() const { return Ld() + npar; }
  KIN_HD double* step() const { return g() + npar; }
  KIN_HD double* p() const { return step() + npar; }
  KIN_HD double* pt() const { return p() + npar; }
  KIN_HD double* e0() const { return pt() + npar; }
  KIN_HD double* e1() const { return e0() + nrow; }
  KIN_HD double* q() const { return e1() + nrow; }                // [HRP_FK_MAX_JOINTS] the evaluation point's joints
  KIN_HD double* pose() const { return q() + HRP_FK_MAX_JOINTS; } // w[3], t[3]
  KIN_HD double* K() const { return pose() + 6; }
  KIN_HD double* T() const { return K() + 9; }                    // [HRP_FK_MAX_JOINTS][12] base-frame pose of every joint's child frame
  KIN_HD double* Xb() const { return T() + 12 * HRP_FK_MAX_JOINTS; }      // [nkp][3] base-frame key-points
  KIN_HD double* xyz() const { return Xb() + 3 * nkp; }
  KIN_HD double* uv() const { return xyz() + 3 * nkp; }
  KIN_HD double* s2() const { return uv() + 2 * nkp; }            // sqrt of the used points' weights, 0 = unused
  KIN_HD double* s3() const { return s2() + nkp; }
  KIN_HD int* pidx() const { return (int*)(s3() + nkp); }         // parameter -> joint column
  KIN_HD int* act() const { return pidx() + npar; }               // held on a bound
  KIN_HD int* bad() const { return act() + npar; }                // a used 2-D point at depth <= 0
  KIN_HD int* anc() const { return bad() + nkp; }                 // [HRP_FK_MAX_JOINTS] ancestors() of every joint
};
KIN_HD size_t shared_doubles(int npar, int nkp, int has3d) {
  const Shared s{nullptr, npar, kin_nrow(nkp, has3d), nkp};
  const size_t doubles = s.jsize() + (size_t)npar * npar + (size_t)npar * (npar + 1) / 2 + 5 * (size_t)npar + 2 * (size_t)s.nrow +
                         HRP_FK_MAX_JOINTS + 6 + 9 + 12 * HRP_FK_MAX_JOINTS + 10 * (size_t)nkp;      // J .. s3, as the accessors lay them out
  return doubles + (2 * (size_t)npar + nkp + HRP_FK_MAX_JOINTS + 1) / 2;                         // pidx, act, bad, anc
}
KIN_HD Shared carve(double* buf, int npar, int nkp, int has3d) { return Shared{buf, npar, kin_nrow(nkp, has3d), nkp}; }

struct Ctx {
  Problem pr;
  Shared sh;
  int npar, nfree, nrow, has3d;
};

KIN_HD double clampq(const Problem& pr, int j, double v) {
  if (pr.q_lo) v = fmax(v, (double)pr.q_lo[j]);
  if (pr.q_hi) v = fmin(v, (double)pr.q_hi[j]);
  return v;
}
KIN_HD double prior_of(const Problem& pr, int j) {
  const double w = pr.prior_q ? (double)pr.prior_q[j] : 0.0;
  return w > 0.0 ? w : 0.0;
}

// rotation of the pose at the evaluation point, and of its re-rooting: X = R (Rr^T (Xb - orr)) + t, Rr = I, orr = 0 for root == 0
struct Camera {
  double R[3][3], t[3], Rr[3][3], orr[3];
};
KIN_HD Camera camera_of(const Ctx& c) {
  const Shared& sh = c.sh;
  Camera C;
  const double w[3] = {sh.pose()[0], sh.pose()[1], sh.pose()[2]};
  rot_aa<double>(w, C.R);      // a fixed pose goes through its angle-axis vector as well (R(log R) is R to a few ulp of fp64)
  for (int a = 0; a < 3; ++a) C.t[a] = sh.pose()[3 + a];
  const int fr = c.pr.root > 0 ? c.pr.ch->kp_frame[c.pr.root] : -1;
  Rigid<double> Tr = rigid_identity<double>();
  if (fr >= 0 && fr < chain_joints(c.pr.ch)) Tr = load12(sh.T() + 12 * fr);
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) C.Rr[a][b] = Tr.r[a][b];
    C.orr[a] = Tr.t[a];
  }
  return C;
}
// Y = Rr^T v (direction) and X = R y
KIN_HD void to_root(const Camera& C, const double (&v)[3], double (&y)[3]) {
  for (int a = 0; a < 3; ++a) y[a] = C.Rr[0][a] * v[0] + C.Rr[1][a] * v[1] + C.Rr[2][a] * v[2];
}
KIN_HD void to_cam(const Camera& C, const double (&y)[3], double (&x)[3]) {
  for (int a = 0; a < 3; ++a) x[a] = C.R[a][0] * y[0] + C.R[a][1] * y[1] + C.R[a][2] * y[2];
}

// the cost at parameter vector pv, its residual rows in e; false when a used 2-D point lies at depth <= 0 or the cost is not finite.
// Leaves the evaluation point in sh.q / sh.pose, the frames in sh.T and the key-points in sh.Xb (base frame), sh.xyz, sh.uv.
//   lane = joint: its local pose (one sin / cos per joint), then its base-frame pose as the product along its ancestors
//   lane = key-point: the point, its projection, its residual rows
template <class Par>
KIN_HD bool evaluate(const Par& par, const Ctx& c, const double* pv, double* e, double& cost) {
  const Shared& sh = c.sh;
  const hrp_fk_chain* ch = c.pr.ch;
  const int nj = chain_joints(ch);
  double* local = sh.J();      // J is spent once M and g are built
  for (int l = par.lo(); l < par.hi(); ++l)
    if (l < c.npar) {
      if (l < c.nfree) sh.q()[sh.pidx()[l]] = pv[l];
      else sh.pose()[l - c.nfree] = pv[l];
    }
  par.sync();
  for (int j = par.lo(); j < par.hi(); ++j)
    if (j < nj) store12(local + 12 * j, joint_local(ch, j, sh.q(), c.pr.dof));
  par.sync();
  for (int j = par.lo(); j < par.hi(); ++j)
    if (j < nj) {
      const uint32_t mask = (uint32_t)sh.anc()[j];
      Rigid<double> T = rigid_identity<double>();
      for (int i = 0; i <= j; ++i)
        if (mask >> i & 1u) T = rigid_mul(T, load12(local + 12 * i));
      store12(sh.T() + 12 * j, T);
    }
  par.sync();
  for (int k = par.lo(); k < par.hi(); ++k)
    if (k < c.pr.nkp) {
      const Camera C = camera_of(c);
      const int f = ch->kp_frame[k];
      const double o[3] = {(double)ch->kp_offset[k][0], (double)ch->kp_offset[k][1], (double)ch->kp_offset[k][2]};
      double Xb[3] = {o[0], o[1], o[2]}, d[3], y[3], X[3], uv[2];
      if (f >= 0 && f < nj) {
        const Rigid<double> T = load12(sh.T() + 12 * f);
        for (int a = 0; a < 3; ++a) Xb[a] = T.r[a][0] * o[0] + T.r[a][1] * o[1] + T.r[a][2] * o[2] + T.t[a];
      }
      for (int a = 0; a < 3; ++a) d[a] = Xb[a] - C.orr[a];
      to_root(C, d, y);
      to_cam(C, y, X);
      for (int a = 0; a < 3; ++a) X[a] += C.t[a];
      project<double>(sh.K(), X, uv);
      for (int a = 0; a < 3; ++a) {
        sh.Xb()[3 * k + a] = Xb[a];
        sh.xyz()[3 * k + a] = X[a];
      }
      sh.uv()[2 * k] = uv[0];
      sh.uv()[2 * k + 1] = uv[1];
      const double s2 = sh.s2()[k];
      e[2 * k] = s2 > 0.0 ? s2 * (uv[0] - (double)c.pr.pts2d[2 * k]) : 0.0;
      e[2 * k + 1] = s2 > 0.0 ? s2 * (uv[1] - (double)c.pr.pts2d[2 * k + 1]) : 0.0;
      sh.bad()[k] = s2 > 0.0 && !(X[2] > 0.0);
      if (c.has3d) {
        const double s3 = sh.s3()[k];
        for (int a = 0; a < 3; ++a)
          e[2 * c.pr.nkp + 3 * k + a] = s3 > 0.0 ? s3 * (X[a] - (double)c.pr.pts3d[3 * k + a]) : 0.0;
      }
    }
  par.sync();
  cost = 0.0;
  bool ok = true;
  for (int r = 0; r < c.nrow; ++r) cost += e[r] * e[r];
  for (int l = 0; l < c.nfree; ++l) {
    const int j = sh.pidx()[l];
    const double w = prior_of(c.pr, j), d = pv[l] - (double)c.pr.q0[j];
    if (w > 0.0) cost += w * d * d;
  }
  for (int k = 0; k < c.pr.nkp; ++k) ok = ok && !sh.bad()[k];
  par.sync();      // e, bad and the evaluation point may be rewritten by the caller's next phase
  return ok && finite64(cost);
}

// J (column l = parameter l, rows as e) at the evaluation point, then M = J^T J + priors and g = J^T e + prior gradient.
// The columns are exact and in closed form from what the evaluation left in sh.T / sh.Xb / sh.xyz:
//   joint column c   sum over the joints j it drives (mimic joints too) of mul_j s_jk v_jk, v_jk = a_j x (Xb_k - p_j) for a revolute and
//                    a_j for a prismatic joint, a_j = T_j.R axis_j and p_j = T_j.t in the base frame; s_jk = [j above key-point k] -
//                    [j above the root key-point] (the second term is the re-rooting's: M = [R | t] T_root^-1); then dX = R Rr^T (sum)
//   w_a              dR/dw_a (rot_aa on a dual number) applied to Rr^T (Xb_k - o_root);    t_a: the unit vector
template <class Par>
KIN_HD void linearise(const Par& par, const Ctx& c, const double* e) {
  const Shared& sh = c.sh;
  const hrp_fk_chain* ch = c.pr.ch;
  const int nkp = c.pr.nkp, nrow = c.nrow, N = c.npar, nj = chain_joints(ch);
  for (int l = par.lo(); l < par.hi(); ++l)
    if (l < N) {
      const Camera C = camera_of(c);
      const int col_q = l < c.nfree ? sh.pidx()[l] : -1, a_pose = l - c.nfree;
      double dR[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
      if (col_q < 0 && a_pose < 3) {
        DD w[3], Rd[3][3];
        for (int a = 0; a < 3; ++a) w[a] = {sh.pose()[a], a == a_pose ? 1.0 : 0.0};
        rot_aa<DD>(w, Rd);
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b) dR[a][b] = Rd[a][b].d;
      }
      const int fr = c.pr.root > 0 ? ch->kp_frame[c.pr.root] : -1;
      const uint32_t above_root = fr >= 0 && fr < nj ? (uint32_t)sh.anc()[fr] : 0u;
      double* col = sh.J() + (size_t)l * nrow;
      for (int k = 0; k < nkp; ++k) {
        const double Xb[3] = {sh.Xb()[3 * k], sh.Xb()[3 * k + 1], sh.Xb()[3 * k + 2]};
        double dX[3] = {0.0, 0.0, 0.0};
        if (col_q >= 0) {
          const int f = ch->kp_frame[k];
          const uint32_t above = f >= 0 && f < nj ? (uint32_t)sh.anc()[f] : 0u;
          double acc[3] = {0.0, 0.0, 0.0}, y[3];
          for (int j = 0; j < nj; ++j) {
            const int s = (int)(above >> j & 1u) - (int)(above_root >> j & 1u);
            if (s == 0 || ch->type[j] == 0 || ch->cfg[j] != col_q) continue;
            const Rigid<double> T = load12(sh.T() + 12 * j);
            const double ax[3] = {(double)ch->axis[j][0], (double)ch->axis[j][1], (double)ch->axis[j][2]};
            double aw[3];
            for (int a = 0; a < 3; ++a) aw[a] = T.r[a][0] * ax[0] + T.r[a][1] * ax[1] + T.r[a][2] * ax[2];
            const double f_ = (double)s * (double)ch->mimic_mul[j];
            if (ch->type[j] == 1) {
              const double r[3] = {Xb[0] - T.t[0], Xb[1] - T.t[1], Xb[2] - T.t[2]};
              acc[0] += f_ * (aw[1] * r[2] - aw[2] * r[1]);
              acc[1] += f_ * (aw[2] * r[0] - aw[0] * r[2]);
              acc[2] += f_ * (aw[0] * r[1] - aw[1] * r[0]);
            } else {
              for (int a = 0; a < 3; ++a) acc[a] += f_ * aw[a];
            }
          }
          to_root(C, acc, y);
          to_cam(C, y, dX);
        } else if (a_pose < 3) {
          const double d[3] = {Xb[0] - C.orr[0], Xb[1] - C.orr[1], Xb[2] - C.orr[2]};
          double y[3];
          to_root(C, d, y);
          for (int a = 0; a < 3; ++a) dX[a] = dR[a][0] * y[0] + dR[a][1] * y[1] + dR[a][2] * y[2];
        } else {
          dX[a_pose - 3] = 1.0;
        }
        // uv = h[:2] / h[2], h = K X
        const double* K = sh.K();
        const double X[3] = {sh.xyz()[3 * k], sh.xyz()[3 * k + 1], sh.xyz()[3 * k + 2]};
        const double h2 = K[6] * X[0] + K[7] * X[1] + K[8] * X[2];
        const double dh0 = K[0] * dX[0] + K[1] * dX[1] + K[2] * dX[2], dh1 = K[3] * dX[0] + K[4] * dX[1] + K[5] * dX[2],
                     dh2 = K[6] * dX[0] + K[7] * dX[1] + K[8] * dX[2];
        const double s2 = sh.s2()[k];
        col[2 * k] = s2 > 0.0 ? s2 * ((dh0 - sh.uv()[2 * k] * dh2) / h2) : 0.0;
        col[2 * k + 1] = s2 > 0.0 ? s2 * ((dh1 - sh.uv()[2 * k + 1] * dh2) / h2) : 0.0;
        if (c.has3d) {
          const double s3 = sh.s3()[k];
          for (int a = 0; a < 3; ++a) col[2 * nkp + 3 * k + a] = s3 > 0.0 ? s3 * dX[a] : 0.0;
        }
      }
    }
  par.sync();
  for (int a = par.lo(); a < par.hi(); ++a)
    if (a < N) {
      const double* ca = sh.J() + (size_t)a * nrow;
      for (int b = a; b < N; ++b) {
        const double* cb = sh.J() + (size_t)b * nrow;
        double s = 0.0;
        for (int r = 0; r < nrow; ++r) s += ca[r] * cb[r];
        sh.M()[a * N + b] = s;
        sh.M()[b * N + a] = s;
      }
      double s = 0.0;
      for (int r = 0; r < nrow; ++r) s += ca[r] * e[r];
      if (a < c.nfree) {
        const int j = sh.pidx()[a];
        const double w = prior_of(c.pr, j);
        sh.M()[a * N + a] += w;
        s += w * (sh.p()[a] - (double)c.pr.q0[j]);
      }
      sh.g()[a] = s;
      // a free joint that sits on a bound while the descent direction -g points across it is held for the next trials
      bool held = false;
      if (a < c.nfree) {
        const int j = sh.pidx()[a];
        held = (c.pr.q_lo && sh.p()[a] <= (double)c.pr.q_lo[j] && s > 0.0) || (c.pr.q_hi && sh.p()[a] >= (double)c.pr.q_hi[j] && s < 0.0);
      }
      sh.act()[a] = held;
    }
  par.sync();
}

KIN_HD double& Lat(const Shared& sh, int r, int c) { return sh.L()[(size_t)r * (r + 1) / 2 + c]; }

// L L^T = M + lambda diag(M), L's diagonal in Ld; false at a pivot that is not positive.  With `hold`, the rows and columns of the
// held joints (sh.act()) are replaced by the identity's: they leave the system.
template <class Par>
KIN_HD bool cholesky(const Par& par, const Ctx& c, double lambda, bool hold) {
  const Shared& sh = c.sh;
  const int N = c.npar;
  for (int r = par.lo(); r < par.hi(); ++r)
    if (r < N)
      for (int k = 0; k <= r; ++k) {
        const double v = sh.M()[r * N + k] + (k == r ? lambda * sh.M()[r * N + r] : 0.0);
        Lat(sh, r, k) = hold && (sh.act()[r] || sh.act()[k]) ? (k == r ? 1.0 : 0.0) : v;
      }
  par.sync();
  for (int k = 0; k < N; ++k) {
    const double d = Lat(sh, k, k);      // final since step k - 1; step k leaves it (its root goes to Ld) and writes below and right of it
    if (!(d > 0.0)) {
      par.sync();
      return false;
    }
    const double sd = sqrt(d);
    for (int r = par.lo(); r < par.hi(); ++r) {
      if (r == k) sh.Ld()[k] = sd;
      if (r > k && r < N) Lat(sh, r, k) = Lat(sh, r, k) / sd;
    }
    par.sync();
    for (int r = par.lo(); r < par.hi(); ++r)
      if (r > k && r < N) {
        const double lrk = Lat(sh, r, k);
        for (int m = k + 1; m <= r; ++m) Lat(sh, r, m) -= lrk * Lat(sh, m, k);
      }
    par.sync();
  }
  return true;
}

// x = (L L^T)^-1 b in place, one lane's work
KIN_HD void chol_apply(const Shared& sh, int N, double* x) {
  for (int r = 0; r < N; ++r) {
    double v = x[r];
    for (int m = 0; m < r; ++m) v -= Lat(sh, r, m) * x[m];
    x[r] = v / sh.Ld()[r];
  }
  for (int r = N - 1; r >= 0; --r) {
    double v = x[r];
    for (int m = r + 1; m < N; ++m) v -= Lat(sh, m, r) * x[m];
    x[r] = v / sh.Ld()[r];
  }
}

template <class Par>
KIN_HD void solve_one(const Par& par, const Problem& pr, double* buf) {
  Ctx c;
  c.pr = pr;
  c.has3d = pr.pts3d && pr.w3d;
  const uint32_t fm = free_mask(pr.free_q, pr.dof);
  c.nfree = popcount32(fm);
  c.npar = c.nfree + (pr.free_pose ? 6 : 0);
  c.nrow = kin_nrow(pr.nkp, c.has3d);
  c.sh = carve(buf, c.npar, pr.nkp, c.has3d);
  const Shared& sh = c.sh;
  const int N = c.npar, nkp = pr.nkp, dof = pr.dof;

  // ---- the start: p, the fixed pose, the usable points ------------------------------------------------------------------------------
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l == 0) {
      double w[3];
      if (pr.rot_dim == 3) {
        for (int a = 0; a < 3; ++a) w[a] = (double)pr.rot0[a];
      } else {
        double r6[6], R[3][3];
        for (int a = 0; a < 6; ++a) r6[a] = (double)pr.rot0[a];
        rot_from_6d(r6, R);
        rot_to_aa(R, w);
      }
      for (int a = 0; a < 3; ++a) {
        sh.pose()[a] = w[a];
        sh.pose()[3 + a] = (double)pr.trans0[a];
      }
    }
    if (l < dof) sh.q()[l] = (double)pr.q0[l];
    if (l < 9) sh.K()[l] = (double)pr.K[l];
    if (l < HRP_FK_MAX_JOINTS) sh.anc()[l] = (int)ancestors(pr.ch, l);
    if (l < nkp) {
      const double w2 = pr.w2d ? (double)pr.w2d[l] : 1.0;
      const bool u2 = w2 > 0.0 && finite64((double)pr.pts2d[2 * l]) && finite64((double)pr.pts2d[2 * l + 1]);
      sh.s2()[l] = u2 ? sqrt(w2) : 0.0;
      bool u3 = false;
      double w3 = 0.0;
      if (c.has3d) {
        w3 = (double)pr.w3d[l];
        u3 = w3 > 0.0 && finite64((double)pr.pts3d[3 * l]) && finite64((double)pr.pts3d[3 * l + 1]) && finite64((double)pr.pts3d[3 * l + 2]);
      }
      sh.s3()[l] = u3 ? sqrt(w3) : 0.0;
    }
    if (l < c.nfree) {
      uint32_t m = fm;
      for (int i = 0; i < l; ++i) m &= m - 1;
      int j = 0;
      while (!(m >> j & 1u)) ++j;
      sh.pidx()[l] = j;
    }
  }
  par.sync();
  for (int l = par.lo(); l < par.hi(); ++l)
    if (l < N) sh.p()[l] = l < c.nfree ? sh.q()[sh.pidx()[l]] : sh.pose()[l - c.nfree];
  par.sync();
  int n2d = 0, n3d = 0, nprior = 0;
  double wsum = 0.0;
  for (int k = 0; k < nkp; ++k) {
    if (sh.s2()[k] > 0.0) {
      ++n2d;
      wsum += pr.w2d ? (double)pr.w2d[k] : 1.0;
    }
    if (sh.s3()[k] > 0.0) ++n3d;
  }
  for (int l = 0; l < c.nfree; ++l) nprior += prior_of(pr, sh.pidx()[l]) > 0.0;
  const int rows = 2 * n2d + 3 * n3d + nprior;

  // ---- lm_refine's loop (pnp.hip), the trial clamped to the joint limits.  One evaluation per pass: of the start (stage 0), of a trial
  // (stage 1), and of the returned parameters (stage 2: the last trial may have been refused, so the evaluation point, the key-points
  // and e are put back at p).  Written as one loop so that the FK code is instantiated once.
  int flags = 0, it = 0, stage = 0, converged = 0;
  double *e = sh.e0(), *et = sh.e1(), cost = 0.0, lambda = 1e-3, smax = 0.0, ymax = 0.0;
  bool solve = false;
  for (;;) {
    const double* pv = stage == 1 ? sh.pt() : sh.p();
    double cn;
    const bool ok = evaluate(par, c, pv, stage == 1 ? et : e, cn);
    if (stage == 2) break;
    bool moved = false, done = false;
    if (stage == 0) {
      cost = cn;
      if (rows < N || N == 0) flags |= HRP_KIN_FEW_ROWS;
      if (!ok) flags |= HRP_KIN_BAD_START;
      solve = flags == 0;
      if (!solve) break;
      moved = true;
    } else {
      if (ok && cn < cost) {
        for (int l = par.lo(); l < par.hi(); ++l)
          if (l < N) sh.p()[l] = sh.pt()[l];
        par.sync();
        double* t = e;
        e = et;
        et = t;
        cost = cn;
        moved = true;
        lambda = fmax(lambda * 0.1, 1e-12);
        if (smax <= 1e-12 * (1.0 + ymax)) converged = 1;
      } else {
        lambda *= 10.0;
        // no step of any length lowers the cost at this precision: the minimum is reached
        if (lambda > 1e10) converged = 1;
      }
      ++it;
      done = converged || it >= KIN_LM_MAX_IT;
    }
    if (moved) linearise(par, c, e);
    // the damped system; a factorisation that fails is a trial that failed
    while (!done && !cholesky(par, c, lambda, true)) {
      lambda *= 10.0;
      ++it;
      if (lambda > 1e10) converged = 1;
      done = converged || it >= KIN_LM_MAX_IT;
    }
    if (done) {
      stage = 2;
      continue;
    }
    for (int l = par.lo(); l < par.hi(); ++l)
      if (l == 0) {
        for (int a = 0; a < N; ++a) sh.step()[a] = sh.act()[a] ? 0.0 : -sh.g()[a];
        chol_apply(sh, N, sh.step());
      }
    par.sync();
    for (int l = par.lo(); l < par.hi(); ++l)
      if (l < N) {
        const double v = sh.p()[l] + sh.step()[l];
        sh.pt()[l] = l < c.nfree ? clampq(pr, sh.pidx()[l], v) : v;
      }
    par.sync();
    smax = ymax = 0.0;
    for (int a = 0; a < N; ++a) {
      smax = fmax(smax, fabs(sh.pt()[a] - sh.p()[a]));
      ymax = fmax(ymax, fabs(sh.p()[a]));
    }
    stage = 1;
  }
  if (solve) {
    if (converged) flags |= HRP_KIN_CONVERGED;
    for (int l = 0; l < c.nfree; ++l) {
      const int j = sh.pidx()[l];
      if ((pr.q_lo && sh.p()[l] == (double)pr.q_lo[j]) || (pr.q_hi && sh.p()[l] == (double)pr.q_hi[j])) flags |= HRP_KIN_AT_LIMIT;
    }
  }

  // ---- outputs -------------------------------------------------------------------------------------------------------------------------
  double ssq = 0.0;
  for (int r = 0; r < 2 * nkp; ++r) ssq += e[r] * e[r];
  bool want_cov = solve && pr.cov && rows > N && !(flags & HRP_KIN_AT_LIMIT);
  if (want_cov) want_cov = cholesky(par, c, 0.0, false);
  if (pr.cov) {
    const double s2 = want_cov ? cost / (double)(rows - N) : 0.0;
    for (int i = par.lo(); i < par.hi(); ++i)
      if (i < N) {
        double* x = sh.J() + (size_t)i * N;      // J is spent
        if (want_cov) {
          for (int r = 0; r < N; ++r) x[r] = r == i ? 1.0 : 0.0;
          chol_apply(sh, N, x);
        }
        for (int r = 0; r < N; ++r) pr.cov[(size_t)i * N + r] = want_cov ? (float)(s2 * x[r]) : 0.f;
      }
  }
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l < dof) pr.q[l] = (solve && (fm >> l & 1u)) ? (float)sh.q()[l] : pr.q0[l];
    if (l < nkp) {
      if (pr.xyz)
        for (int a = 0; a < 3; ++a) pr.xyz[3 * l + a] = (float)sh.xyz()[3 * l + a];
      if (pr.uv) {
        pr.uv[2 * l] = (float)sh.uv()[2 * l];
        pr.uv[2 * l + 1] = (float)sh.uv()[2 * l + 1];
      }
    }
    if (l == 0) {
      if (solve && pr.free_pose) {
        double w[3] = {sh.pose()[0], sh.pose()[1], sh.pose()[2]};
        const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (th > M_PI) {      // pnp_lm.h's normalise_rotation
          double tn = fmod(th, 2.0 * M_PI);
          if (tn > M_PI) tn -= 2.0 * M_PI;
          for (int a = 0; a < 3; ++a) w[a] *= tn / th;
        }
        if (pr.rot_dim == 3) {
          for (int a = 0; a < 3; ++a) pr.rot[a] = (float)w[a];
        } else {
          double R[3][3];
          rot_aa<double>(w, R);
          for (int a = 0; a < 6; ++a) pr.rot[a] = (float)R[a / 3][a % 3];
        }
        for (int a = 0; a < 3; ++a) pr.trans[a] = (float)sh.pose()[3 + a];
      } else {
        for (int a = 0; a < pr.rot_dim; ++a) pr.rot[a] = pr.rot0[a];
        for (int a = 0; a < 3; ++a) pr.trans[a] = pr.trans0[a];
      }
      if (pr.rms) pr.rms[0] = wsum > 0.0 ? (float)sqrt(ssq / wsum) : 0.f;
      if (pr.status) {
        pr.status[0] = flags;
        pr.status[1] = it;
        pr.status[2] = rows;
        pr.status[3] = N;
      }
    }
  }
}

// the descriptor's pointers narrowed to sample b
KIN_HD Problem problem_of(const hrp_kin_desc& d, int b) {
  const int nkp = d.nkp, dof = d.dof;
  const int npar = kin_npar(d.free_q, dof, d.free_pose);
  const size_t bp = d.pose_stride ? (size_t)b : 0;
  Problem p;
  p.ch = d.chain;
  p.pts2d = d.pts2d + (size_t)b * nkp * 2;
  p.w2d = d.w2d ? d.w2d + (size_t)b * nkp : nullptr;
  p.pts3d = d.pts3d ? d.pts3d + (size_t)b * nkp * 3 : nullptr;
  p.w3d = d.w3d ? d.w3d + (size_t)b * nkp : nullptr;
  p.K = d.K + (size_t)b * d.K_stride;
  p.q0 = d.q0 + (size_t)b * dof;
  p.rot0 = d.rot0 + bp * d.rot_dim;
  p.trans0 = d.trans0 + bp * 3;
  p.q_lo = d.q_lo;
  p.q_hi = d.q_hi;
  p.prior_q = d.prior_q;
  p.nkp = nkp;
  p.dof = dof;
  p.rot_dim = d.rot_dim;
  p.free_pose = d.free_pose;
  p.root = d.root;
  p.free_q = d.free_q;
  p.q = d.q + (size_t)b * dof;
  p.rot = d.rot + (size_t)b * d.rot_dim;
  p.trans = d.trans + (size_t)b * 3;
  p.xyz = d.xyz ? d.xyz + (size_t)b * nkp * 3 : nullptr;
  p.uv = d.uv ? d.uv + (size_t)b * nkp * 2 : nullptr;
  p.rms = d.rms ? d.rms + b : nullptr;
  p.status = d.status ? d.status + (size_t)b * 4 : nullptr;
  p.cov = d.cov ? d.cov + (size_t)b * npar * npar : nullptr;
  return p;
}

// what hrp_kin_solve refuses, as a text (NULL: the descriptor is usable)
KIN_HD const char* refusal(const hrp_kin_desc* d) {
  if (!d) return "null descriptor";
  if (!d->chain || !d->pts2d || !d->K || !d->rot0 || !d->trans0 || !d->rot || !d->trans) return "null required pointer";
  if (d->dof > 0 && (!d->q0 || !d->q)) return "null required pointer (q0, q)";
  if (d->B <= 0) return "B <= 0";
  if (d->rot_dim != 3 && d->rot_dim != 6) return "rot_dim (3 or 6)";
  if (d->nkp < 1 || d->nkp > HRP_FK_MAX_KP) return "nkp (1..HRP_FK_MAX_KP)";
  if (d->dof < 0 || d->dof > HRP_FK_MAX_JOINTS) return "dof (0..HRP_FK_MAX_JOINTS)";
  if (d->free_q != free_mask(d->free_q, d->dof)) return "free_q has a bit at or above dof";
  if ((d->pts3d != nullptr) != (d->w3d != nullptr)) return "pts3d and w3d go together";
  if (d->K_stride != 0 && d->K_stride != 9) return "K_stride (0 or 9)";
  if (d->pose_stride != 0 && d->pose_stride != 1) return "pose_stride (0 or 1)";
  if (d->free_pose != 0 && d->free_pose != 1) return "free_pose (0 or 1)";
  if (d->root < 0 || d->root >= d->nkp) return "root (0..nkp-1)";
  return nullptr;
}

}  // namespace kin
}  // namespace hrp
