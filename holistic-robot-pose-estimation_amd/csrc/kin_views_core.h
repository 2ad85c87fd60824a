// The multi-view kinematic refit (hrp_kin_solve_views, include/hrp.h): Levenberg-Marquardt on the free joint angles of one sample over
// the 2-D key-points seen by V fixed, calibrated cameras and a prior on the joints.  It is kin_core.h's loop (hrp_kin_solve with
// free_pose = 0, root = 0) with the residual rows of V views stacked, written once for the kernel of kin_views.hip (one 64-lane
// workgroup per sample) and for a host compiler (tests/kinviews_host_check.cpp) behind kin_core.h's `Par` policy.  kin_core.h's pieces
// are called as they stand: joint_local, ancestors, rot_aa, project, cholesky, chol_apply, clampq, prior_of and the Shared layout, which
// is carved for ONE view's rows; what V views add lies behind it in `Views`.
//
//   value phase      the forward kinematics ONCE per evaluation - lane = joint: its local pose (one sin / cos pair), then its base-frame
//                    pose; lane = key-point: the base-frame point - then lane = (view, key-point) pair, in steps of 64: the camera point
//                    R(w_v) Xb_k + t_v, its projection, its residual rows
//   Jacobian phase   lane = parameter: the base-frame column a_j x (Xb_k - p_j) of every key-point, which no view changes, once into LDS;
//                    then view after view, lane = parameter: that column rotated by R(w_v) and pushed through the projection's 2 x 3
//                    derivative into J_v [npar][2 nkp], and lane = row a: J_v^T J_v and J_v^T e_v added into M and g.  Only one view's
//                    Jacobian is ever held.  A view without a used point is passed over (its rows are zeros).
//   sums             views ascending, then kin_core.h's row order; every decision is taken from shared values.
#pragma once
#include "kin_core.h"

namespace hrp {
namespace kinv {

using kin::KIN_LANES;
using kin::Shared;

// One sample.  `k` is kin_core.h's Problem with the 2-D arrays carrying V views: pts2d [V][nkp][2], w2d [V][nkp], K [V][9], xyz
// [V][nkp][3], uv [V][nkp][2]; its pts3d, w3d, rot0, trans0, rot, trans are NULL and free_pose, root are 0.
struct Problem {
  kin::Problem k;
  const float* poses;      // [V][6] camera-from-base, angle-axis then translation
  int V;
  float* rms_view;         // [V]
  int32_t* used_view;      // [V]
};

// What V views keep in LDS behind kin_core.h's Shared (which holds one view's J, M, L, g, the parameters, the frames and Xb).
struct Views {
  double* base;
  int npar, nkp, V;
  KIN_HD double* e() const { return base; }                                   // [V][2 nkp] residual rows of the last evaluation
  KIN_HD double* uv() const { return e() + 2 * (size_t)V * nkp; }             // [V][nkp][2]
  KIN_HD double* h2() const { return uv() + 2 * (size_t)V * nkp; }            // [V][nkp] (K X)[2]
  KIN_HD double* s2() const { return h2() + (size_t)V * nkp; }                // [V][nkp] sqrt of the used points' weights, 0 = unused
  KIN_HD double* Rt() const { return s2() + (size_t)V * nkp; }                // [V][12] rows of [R(w_v) | t_v]
  KIN_HD double* K() const { return Rt() + 12 * (size_t)V; }                  // [V][9]
  KIN_HD double* Jb() const { return K() + 9 * (size_t)V; }                   // [npar][nkp][3] base-frame columns
  KIN_HD int* bad() const { return (int*)(Jb() + 3 * (size_t)npar * nkp); }   // [V][nkp] a used point at depth <= 0
  KIN_HD int* used() const { return bad() + (size_t)V * nkp; }                // [V] used points of the view
};
KIN_HD size_t views_doubles(int npar, int nkp, int V) {
  return 6 * (size_t)V * nkp + 21 * (size_t)V + 3 * (size_t)npar * nkp + ((size_t)V * nkp + V + 1) / 2;
}
KIN_HD size_t shared_doubles(int npar, int nkp, int V) { return kin::shared_doubles(npar, nkp, 0) + views_doubles(npar, nkp, V); }

struct Ctx {
  kin::Ctx k;      // pr, sh (one view's rows), npar = nfree, nrow = 2 nkp, has3d = 0
  Views vw;
  int V;
};

// the cost at parameter vector pv, its residual rows in vw.e; false when a used point of any view lies at depth <= 0 or the cost is not
// finite.  Leaves the evaluation point in sh.q, the frames in sh.T, the base-frame key-points in sh.Xb and every view's uv and h2.
template <class Par>
KIN_HD bool evaluate(const Par& par, const Ctx& c, const double* pv, double& cost) {
  const Shared& sh = c.k.sh;
  const Views& vw = c.vw;
  const kin::Problem& pr = c.k.pr;
  const hrp_fk_chain* ch = pr.ch;
  const int nj = kin::chain_joints(ch), nkp = pr.nkp, N = c.k.npar, npair = c.V * nkp;
  double* local = sh.J();      // J_v is spent once M and g are built
  for (int l = par.lo(); l < par.hi(); ++l)
    if (l < N) sh.q()[sh.pidx()[l]] = pv[l];
  par.sync();
  for (int j = par.lo(); j < par.hi(); ++j)
    if (j < nj) kin::store12(local + 12 * j, kin::joint_local(ch, j, sh.q(), pr.dof));
  par.sync();
  for (int j = par.lo(); j < par.hi(); ++j)
    if (j < nj) {
      const uint32_t mask = (uint32_t)sh.anc()[j];
      kin::Rigid<double> T = kin::rigid_identity<double>();
      for (int i = 0; i <= j; ++i)
        if (mask >> i & 1u) T = kin::rigid_mul(T, kin::load12(local + 12 * i));
      kin::store12(sh.T() + 12 * j, T);
    }
  par.sync();
  for (int k = par.lo(); k < par.hi(); ++k)
    if (k < nkp) {
      const int f = ch->kp_frame[k];
      const double o[3] = {(double)ch->kp_offset[k][0], (double)ch->kp_offset[k][1], (double)ch->kp_offset[k][2]};
      double Xb[3] = {o[0], o[1], o[2]};
      if (f >= 0 && f < nj) {
        const kin::Rigid<double> T = kin::load12(sh.T() + 12 * f);
        for (int a = 0; a < 3; ++a) Xb[a] = T.r[a][0] * o[0] + T.r[a][1] * o[1] + T.r[a][2] * o[2] + T.t[a];
      }
      for (int a = 0; a < 3; ++a) sh.Xb()[3 * k + a] = Xb[a];
    }
  par.sync();
  for (int i0 = 0; i0 < npair; i0 += KIN_LANES)
    for (int l = par.lo(); l < par.hi(); ++l) {
      const int i = i0 + l;
      if (i >= npair) continue;
      const int v = i / nkp, k = i - v * nkp;
      const kin::Rigid<double> C = kin::load12(vw.Rt() + 12 * v);
      const double* K = vw.K() + 9 * v;
      const double Xb[3] = {sh.Xb()[3 * k], sh.Xb()[3 * k + 1], sh.Xb()[3 * k + 2]};
      double X[3], uv[2];
      for (int a = 0; a < 3; ++a) X[a] = C.r[a][0] * Xb[0] + C.r[a][1] * Xb[1] + C.r[a][2] * Xb[2] + C.t[a];
      kin::project<double>(K, X, uv);
      vw.uv()[2 * i] = uv[0];
      vw.uv()[2 * i + 1] = uv[1];
      vw.h2()[i] = K[6] * X[0] + K[7] * X[1] + K[8] * X[2];
      const double s2 = vw.s2()[i];
      vw.e()[2 * i] = s2 > 0.0 ? s2 * (uv[0] - (double)pr.pts2d[2 * i]) : 0.0;
      vw.e()[2 * i + 1] = s2 > 0.0 ? s2 * (uv[1] - (double)pr.pts2d[2 * i + 1]) : 0.0;
      vw.bad()[i] = s2 > 0.0 && !(X[2] > 0.0);
    }
  par.sync();
  cost = 0.0;
  bool ok = true;
  for (int r = 0; r < 2 * npair; ++r) cost += vw.e()[r] * vw.e()[r];
  for (int l = 0; l < N; ++l) {
    const int j = sh.pidx()[l];
    const double w = kin::prior_of(pr, j), d = pv[l] - (double)pr.q0[j];
    if (w > 0.0) cost += w * d * d;
  }
  for (int i = 0; i < npair; ++i) ok = ok && !vw.bad()[i];
  par.sync();      // e, bad and the evaluation point may be rewritten by the caller's next phase
  return ok && kin::finite64(cost);
}

// M = sum_v J_v^T J_v + priors and g = sum_v J_v^T e_v + prior gradient at the evaluation point, from what the evaluation left in
// sh.T / sh.Xb / vw.uv / vw.h2.  The joint column is kin_core.h's with root == 0: the sum over the joints j it drives (mimic joints
// too) of mul_j [j above key-point k] v_jk, v_jk = a_j x (Xb_k - p_j) for a revolute and a_j for a prismatic joint.
template <class Par>
KIN_HD void linearise(const Par& par, const Ctx& c) {
  const Shared& sh = c.k.sh;
  const Views& vw = c.vw;
  const kin::Problem& pr = c.k.pr;
  const hrp_fk_chain* ch = pr.ch;
  const int nkp = pr.nkp, nrow = 2 * nkp, N = c.k.npar, nj = kin::chain_joints(ch);
  for (int l = par.lo(); l < par.hi(); ++l)
    if (l < N) {
      const int col_q = sh.pidx()[l];
      double* jb = vw.Jb() + 3 * (size_t)l * nkp;
      for (int k = 0; k < nkp; ++k) {
        const double Xb[3] = {sh.Xb()[3 * k], sh.Xb()[3 * k + 1], sh.Xb()[3 * k + 2]};
        const int f = ch->kp_frame[k];
        const uint32_t above = f >= 0 && f < nj ? (uint32_t)sh.anc()[f] : 0u;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < nj; ++j) {
          if (!(above >> j & 1u) || ch->type[j] == 0 || ch->cfg[j] != col_q) continue;
          const kin::Rigid<double> T = kin::load12(sh.T() + 12 * j);
          const double ax[3] = {(double)ch->axis[j][0], (double)ch->axis[j][1], (double)ch->axis[j][2]};
          double aw[3];
          for (int a = 0; a < 3; ++a) aw[a] = T.r[a][0] * ax[0] + T.r[a][1] * ax[1] + T.r[a][2] * ax[2];
          const double f_ = (double)ch->mimic_mul[j];
          if (ch->type[j] == 1) {
            const double r[3] = {Xb[0] - T.t[0], Xb[1] - T.t[1], Xb[2] - T.t[2]};
            acc[0] += f_ * (aw[1] * r[2] - aw[2] * r[1]);
            acc[1] += f_ * (aw[2] * r[0] - aw[0] * r[2]);
            acc[2] += f_ * (aw[0] * r[1] - aw[1] * r[0]);
          } else {
            for (int a = 0; a < 3; ++a) acc[a] += f_ * aw[a];
          }
        }
        for (int a = 0; a < 3; ++a) jb[3 * k + a] = acc[a];
      }
    }
  par.sync();
  bool first = true;
  for (int v = 0; v < c.V; ++v) {
    if (vw.used()[v] == 0) continue;      // a shared value: every lane passes over the same views
    for (int l = par.lo(); l < par.hi(); ++l)
      if (l < N) {
        const kin::Rigid<double> C = kin::load12(vw.Rt() + 12 * v);
        const double* K = vw.K() + 9 * v;
        const double* jb = vw.Jb() + 3 * (size_t)l * nkp;
        double* col = sh.J() + (size_t)l * nrow;
        for (int k = 0; k < nkp; ++k) {
          const int i = v * nkp + k;
          double dX[3];
          for (int a = 0; a < 3; ++a) dX[a] = C.r[a][0] * jb[3 * k] + C.r[a][1] * jb[3 * k + 1] + C.r[a][2] * jb[3 * k + 2];
          // uv = h[:2] / h[2], h = K X
          const double h2 = vw.h2()[i];
          const double dh0 = K[0] * dX[0] + K[1] * dX[1] + K[2] * dX[2], dh1 = K[3] * dX[0] + K[4] * dX[1] + K[5] * dX[2],
                       dh2 = K[6] * dX[0] + K[7] * dX[1] + K[8] * dX[2];
          const double s2 = vw.s2()[i];
          col[2 * k] = s2 > 0.0 ? s2 * ((dh0 - vw.uv()[2 * i] * dh2) / h2) : 0.0;
          col[2 * k + 1] = s2 > 0.0 ? s2 * ((dh1 - vw.uv()[2 * i + 1] * dh2) / h2) : 0.0;
        }
      }
    par.sync();
    const double* e = vw.e() + (size_t)v * nrow;
    for (int a = par.lo(); a < par.hi(); ++a)
      if (a < N) {
        const double* ca = sh.J() + (size_t)a * nrow;
        for (int b = a; b < N; ++b) {      // the upper triangle carries the running sums; entry (a, b >= a) is lane a's alone
          const double* cb = sh.J() + (size_t)b * nrow;
          double s = first ? 0.0 : sh.M()[a * N + b];
          for (int r = 0; r < nrow; ++r) s += ca[r] * cb[r];
          sh.M()[a * N + b] = s;
        }
        double s = first ? 0.0 : sh.g()[a];
        for (int r = 0; r < nrow; ++r) s += ca[r] * e[r];
        sh.g()[a] = s;
      }
    par.sync();      // the next view writes J_v again
    first = false;
  }
  for (int a = par.lo(); a < par.hi(); ++a)
    if (a < N) {
      if (first) {
        for (int b = a; b < N; ++b) sh.M()[a * N + b] = 0.0;
        sh.g()[a] = 0.0;
      }
      for (int b = a + 1; b < N; ++b) sh.M()[b * N + a] = sh.M()[a * N + b];
      const int j = sh.pidx()[a];
      const double w = kin::prior_of(pr, j);
      const double s = sh.g()[a] + w * (sh.p()[a] - (double)pr.q0[j]);
      sh.M()[a * N + a] += w;
      sh.g()[a] = s;
      // a free joint that sits on a bound while the descent direction -g points across it is held for the next trials
      sh.act()[a] = (pr.q_lo && sh.p()[a] <= (double)pr.q_lo[j] && s > 0.0) || (pr.q_hi && sh.p()[a] >= (double)pr.q_hi[j] && s < 0.0);
    }
  par.sync();
}

template <class Par>
KIN_HD void solve_one(const Par& par, const Problem& vp, double* buf) {
  const kin::Problem& pr = vp.k;
  Ctx c;
  c.k.pr = pr;
  c.k.has3d = 0;
  const uint32_t fm = kin::free_mask(pr.free_q, pr.dof);
  c.k.nfree = c.k.npar = kin::popcount32(fm);
  c.k.nrow = kin::kin_nrow(pr.nkp, 0);
  c.k.sh = kin::carve(buf, c.k.npar, pr.nkp, 0);
  c.V = vp.V;
  c.vw = Views{buf + kin::shared_doubles(c.k.npar, pr.nkp, 0), c.k.npar, pr.nkp, vp.V};
  const Shared& sh = c.k.sh;
  const Views& vw = c.vw;
  const int N = c.k.npar, nkp = pr.nkp, dof = pr.dof, V = vp.V, npair = V * nkp;

  // ---- the start: p, the views' poses and intrinsics, the usable points ------------------------------------------------------------
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l < V) {
      const double w[3] = {(double)vp.poses[6 * l], (double)vp.poses[6 * l + 1], (double)vp.poses[6 * l + 2]};
      kin::Rigid<double> C;
      kin::rot_aa<double>(w, C.r);
      for (int a = 0; a < 3; ++a) C.t[a] = (double)vp.poses[6 * l + 3 + a];
      kin::store12(vw.Rt() + 12 * l, C);
      for (int a = 0; a < 9; ++a) vw.K()[9 * l + a] = (double)pr.K[9 * l + a];
    }
    if (l < dof) sh.q()[l] = (double)pr.q0[l];
    if (l < HRP_FK_MAX_JOINTS) sh.anc()[l] = (int)kin::ancestors(pr.ch, l);
    if (l < N) {
      uint32_t m = fm;
      for (int i = 0; i < l; ++i) m &= m - 1;
      int j = 0;
      while (!(m >> j & 1u)) ++j;
      sh.pidx()[l] = j;
    }
  }
  for (int i0 = 0; i0 < npair; i0 += KIN_LANES)
    for (int l = par.lo(); l < par.hi(); ++l) {
      const int i = i0 + l;
      if (i >= npair) continue;
      const double w2 = pr.w2d ? (double)pr.w2d[i] : 1.0;
      const bool u2 = w2 > 0.0 && kin::finite64((double)pr.pts2d[2 * i]) && kin::finite64((double)pr.pts2d[2 * i + 1]);
      vw.s2()[i] = u2 ? sqrt(w2) : 0.0;
    }
  par.sync();
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l < N) sh.p()[l] = sh.q()[sh.pidx()[l]];
    if (l < V) {
      int n = 0;
      for (int k = 0; k < nkp; ++k) n += vw.s2()[l * nkp + k] > 0.0;
      vw.used()[l] = n;
    }
  }
  par.sync();
  int n2d = 0, nprior = 0;
  for (int v = 0; v < V; ++v) n2d += vw.used()[v];
  for (int l = 0; l < N; ++l) nprior += kin::prior_of(pr, sh.pidx()[l]) > 0.0;
  const int rows = 2 * n2d + nprior;

  // ---- kin_core.h's loop.  One evaluation per pass: of the start (stage 0), of a trial (stage 1), and of the returned parameters
  // (stage 2: the last trial may have been refused).  The residual rows are read only right after an evaluation that was accepted - by
  // the linearisation - and after stage 2, so one buffer serves: a refused trial may leave its rows there.
  int flags = 0, it = 0, stage = 0, converged = 0;
  double cost = 0.0, lambda = 1e-3, smax = 0.0, ymax = 0.0;
  bool solve = false;
  for (;;) {
    const double* pv = stage == 1 ? sh.pt() : sh.p();
    double cn;
    const bool ok = evaluate(par, c, pv, cn);
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
      done = converged || it >= kin::KIN_LM_MAX_IT;
    }
    if (moved) linearise(par, c);
    // the damped system; a factorisation that fails is a trial that failed
    while (!done && !kin::cholesky(par, c.k, lambda, true)) {
      lambda *= 10.0;
      ++it;
      if (lambda > 1e10) converged = 1;
      done = converged || it >= kin::KIN_LM_MAX_IT;
    }
    if (done) {
      stage = 2;
      continue;
    }
    for (int l = par.lo(); l < par.hi(); ++l)
      if (l == 0) {
        for (int a = 0; a < N; ++a) sh.step()[a] = sh.act()[a] ? 0.0 : -sh.g()[a];
        kin::chol_apply(sh, N, sh.step());
      }
    par.sync();
    for (int l = par.lo(); l < par.hi(); ++l)
      if (l < N) sh.pt()[l] = kin::clampq(pr, sh.pidx()[l], sh.p()[l] + sh.step()[l]);
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
    for (int l = 0; l < N; ++l) {
      const int j = sh.pidx()[l];
      if ((pr.q_lo && sh.p()[l] == (double)pr.q_lo[j]) || (pr.q_hi && sh.p()[l] == (double)pr.q_hi[j])) flags |= HRP_KIN_AT_LIMIT;
    }
  }

  // ---- outputs -------------------------------------------------------------------------------------------------------------------------
  bool want_cov = solve && pr.cov && rows > N && !(flags & HRP_KIN_AT_LIMIT);
  if (want_cov) want_cov = kin::cholesky(par, c.k, 0.0, false);
  if (pr.cov) {
    const double s2 = want_cov ? cost / (double)(rows - N) : 0.0;
    for (int i = par.lo(); i < par.hi(); ++i)
      if (i < N) {
        double* x = sh.J() + (size_t)i * N;      // J_v is spent
        if (want_cov) {
          for (int r = 0; r < N; ++r) x[r] = r == i ? 1.0 : 0.0;
          kin::chol_apply(sh, N, x);
        }
        for (int r = 0; r < N; ++r) pr.cov[(size_t)i * N + r] = want_cov ? (float)(s2 * x[r]) : 0.f;
      }
  }
  for (int i0 = 0; i0 < npair; i0 += KIN_LANES)
    for (int l = par.lo(); l < par.hi(); ++l) {
      const int i = i0 + l;
      if (i >= npair) continue;
      const int v = i / nkp, k = i - v * nkp;
      if (pr.xyz) {
        const kin::Rigid<double> C = kin::load12(vw.Rt() + 12 * v);
        const double Xb[3] = {sh.Xb()[3 * k], sh.Xb()[3 * k + 1], sh.Xb()[3 * k + 2]};
        for (int a = 0; a < 3; ++a) pr.xyz[3 * i + a] = (float)(C.r[a][0] * Xb[0] + C.r[a][1] * Xb[1] + C.r[a][2] * Xb[2] + C.t[a]);
      }
      if (pr.uv) {
        pr.uv[2 * i] = (float)vw.uv()[2 * i];
        pr.uv[2 * i + 1] = (float)vw.uv()[2 * i + 1];
      }
    }
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l < dof) pr.q[l] = (solve && (fm >> l & 1u)) ? (float)sh.q()[l] : pr.q0[l];
    if (l < V) {
      double ssq = 0.0, wsum = 0.0;
      for (int k = 0; k < nkp; ++k) {
        const int i = l * nkp + k;
        ssq += vw.e()[2 * i] * vw.e()[2 * i] + vw.e()[2 * i + 1] * vw.e()[2 * i + 1];
        if (vw.s2()[i] > 0.0) wsum += pr.w2d ? (double)pr.w2d[i] : 1.0;
      }
      if (vp.rms_view) vp.rms_view[l] = wsum > 0.0 ? (float)sqrt(ssq / wsum) : 0.f;
      if (vp.used_view) vp.used_view[l] = vw.used()[l];
    }
    if (l == 0) {
      double ssq = 0.0, wsum = 0.0;
      for (int i = 0; i < npair; ++i) {
        ssq += vw.e()[2 * i] * vw.e()[2 * i] + vw.e()[2 * i + 1] * vw.e()[2 * i + 1];
        if (vw.s2()[i] > 0.0) wsum += pr.w2d ? (double)pr.w2d[i] : 1.0;
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
KIN_HD Problem problem_of(const hrp_kin_views_desc& d, int b) {
  const int nkp = d.nkp, dof = d.dof, V = d.V;
  const int npar = kin::kin_npar(d.free_q, dof, 0);
  const size_t pairs = (size_t)b * V * nkp;
  Problem p;
  p.k.ch = d.chain;
  p.k.pts2d = d.pts2d + pairs * 2;
  p.k.w2d = d.w2d ? d.w2d + pairs : nullptr;
  p.k.pts3d = p.k.w3d = nullptr;
  p.k.K = d.K + (d.K_stride ? (size_t)b * V * 9 : 0);
  p.k.q0 = d.q0 + (size_t)b * dof;
  p.k.rot0 = p.k.trans0 = nullptr;
  p.k.q_lo = d.q_lo;
  p.k.q_hi = d.q_hi;
  p.k.prior_q = d.prior_q;
  p.k.nkp = nkp;
  p.k.dof = dof;
  p.k.rot_dim = 3;
  p.k.free_pose = 0;
  p.k.root = 0;
  p.k.free_q = d.free_q;
  p.k.q = d.q + (size_t)b * dof;
  p.k.rot = p.k.trans = nullptr;
  p.k.xyz = d.xyz ? d.xyz + pairs * 3 : nullptr;
  p.k.uv = d.uv ? d.uv + pairs * 2 : nullptr;
  p.k.rms = d.rms ? d.rms + b : nullptr;
  p.k.status = d.status ? d.status + (size_t)b * 4 : nullptr;
  p.k.cov = d.cov ? d.cov + (size_t)b * npar * npar : nullptr;
  p.poses = d.poses + (d.pose_stride ? (size_t)b * V * 6 : 0);
  p.V = V;
  p.rms_view = d.rms_view ? d.rms_view + (size_t)b * V : nullptr;
  p.used_view = d.used_view ? d.used_view + (size_t)b * V : nullptr;
  return p;
}

// what hrp_kin_solve_views refuses, as a text (NULL: the descriptor is usable)
KIN_HD const char* refusal(const hrp_kin_views_desc* d) {
  if (!d) return "null descriptor";
  if (!d->chain || !d->pts2d || !d->K || !d->poses) return "null required pointer";
  if (d->dof > 0 && (!d->q0 || !d->q)) return "null required pointer (q0, q)";
  if (d->B <= 0) return "B <= 0";
  if (d->V < 1 || d->V > HRP_KIN_MAX_VIEWS) return "V (1..HRP_KIN_MAX_VIEWS)";
  if (d->nkp < 1 || d->nkp > HRP_FK_MAX_KP) return "nkp (1..HRP_FK_MAX_KP)";
  if (d->dof < 0 || d->dof > HRP_FK_MAX_JOINTS) return "dof (0..HRP_FK_MAX_JOINTS)";
  if (d->free_q != kin::free_mask(d->free_q, d->dof)) return "free_q has a bit at or above dof";
  if (d->K_stride != 0 && d->K_stride != 9) return "K_stride (0 or 9)";
  if (d->pose_stride != 0 && d->pose_stride != 1) return "pose_stride (0 or 1)";
  if (shared_doubles(kin::kin_npar(d->free_q, d->dof, 0), d->nkp, d->V) * sizeof(double) > 64 * 1024) return "more than 64 KB of LDS";
  return nullptr;
}

}  // namespace kinv
}  // namespace hrp
