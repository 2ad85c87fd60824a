// The kinematic filter (hrp_kin_filter_step, include/hrp.h): one frame of an iterated extended Kalman filter in information form on
// hrp_kin_solve's parameter vector, with a constant-velocity prior and an innovation gate.  Like kin_core.h it is written once for the
// kernel of kin_filter.hip (one 64-lane workgroup per stream) and for a host compiler (tests/kinfilter_host_check.cpp), through the same
// `Par` policy, and it uses kin_core.h as it stands: evaluate (FK, projection, residual rows), linearise (closed-form Jacobian columns,
// J^T J, J^T e, the held joints), cholesky and chol_apply are called, not copied, and kin_core.h is not changed, so hrp_kin_solve keeps
// its code.  The dense prior (p - p-)^T A^-1 (p - p-) is added here, after those calls: to the cost after evaluate, to M, g and the held
// joints after linearise.  The joints' direct measurement (w_q, q_meas) is kin_core.h's own prior term: Problem.prior_q = w_q and
// Problem.q0 = a copy of q_meas staged in LDS (0 where w_q is not positive, so that nothing unread reaches the sums).
//
//   state       mean (p, v) and cov [2n][2n] in global memory, fp64, read at the start of the step and written at its end
//   LDS         kin_core.h's Shared (has3d = 0), then Extra: A, B, C (the predicted blocks), A^-1, A+, G, p-, v-, v+, ...
//   lane        = parameter (a row of every matrix), = key-point (usable, gate statistic), = joint (inside evaluate)
// Every decision is taken from shared values, identically in each lane, and every sum runs in index order.
#pragma once
#include "kin_core.h"

namespace hrp {
namespace kinf {

using kin::Ctx;
using kin::Problem;
using kin::Shared;
using kin::finite64;

constexpr int MAX_N = HRP_KIN_FILTER_MAX_N;

struct Stream {      // this stream's pointers and the launch's scalars
  Problem pr;        // what kin_core.h reads and the fp32 outputs q, rot, trans, xyz, uv, status; q0 is set by step_one
  const float *q_in, *rot_in, *trans_in, *q_meas;
  const int32_t* keep;
  const double *q_acc, *p0_var;
  double dt, gate;
  int max_coast;
  double *mean, *cov;
  int32_t *valid, *coast;
  float *vel, *cov_p, *xyz_next, *d2;
};

// the filter's own shared arrays, behind kin_core.h's
struct Extra {
  double* base;
  int N, nkp, dof;
  KIN_HD size_t NN() const { return (size_t)N * N; }
  KIN_HD double* A() const { return base; }               // P-_pp; A - A+ once A+ is known
  KIN_HD double* Bm() const { return A() + NN(); }        // P-_vp; G (A - A+) once G is known
  KIN_HD double* Cm() const { return Bm() + NN(); }       // P-_vv; P+_vv at the end
  KIN_HD double* Ai() const { return Cm() + NN(); }       // A^-1; G A+ once G is known
  KIN_HD double* Ap() const { return Ai() + NN(); }       // A+ = M^-1
  KIN_HD double* G() const { return Ap() + NN(); }        // B A^-1
  KIN_HD double* pm() const { return G() + NN(); }        // p-
  KIN_HD double* vm() const { return pm() + N; }          // v-
  KIN_HD double* vp() const { return vm() + N; }          // v+
  KIN_HD double* tmp() const { return vp() + N; }
  KIN_HD double* pin() const { return tmp() + N; }        // the inputs as a parameter vector
  KIN_HD double* d2() const { return pin() + N; }         // [nkp] gate statistics, NaN = none
  KIN_HD double* su() const { return d2() + nkp; }        // [nkp] sqrt of the usable points' weights, before the gate
  KIN_HD float* q0s() const { return (float*)(su() + nkp); }      // [dof] q_meas where w_q > 0, else 0
};
KIN_HD size_t extra_doubles(int N, int nkp, int dof) { return 6 * (size_t)N * N + 5 * (size_t)N + 2 * (size_t)nkp + ((size_t)dof + 1) / 2; }
KIN_HD size_t shared_doubles(int N, int nkp, int dof) { return kin::shared_doubles(N, nkp, 0) + extra_doubles(N, nkp, dof); }

// (pv - p-)^T A^-1 (pv - p-): lane = row, then the rows' terms in index order
template <class Par>
KIN_HD double prior_cost(const Par& par, const Extra& x, const double* pv) {
  const int N = x.N;
  for (int a = par.lo(); a < par.hi(); ++a)
    if (a < N) {
      double s = 0.0;
      for (int b = 0; b < N; ++b) s += x.Ai()[(size_t)a * N + b] * (pv[b] - x.pm()[b]);
      x.tmp()[a] = (pv[a] - x.pm()[a]) * s;
    }
  par.sync();
  double s = 0.0;
  for (int a = 0; a < N; ++a) s += x.tmp()[a];
  par.sync();
  return s;
}

// kin_core.h's evaluate plus the dense prior
template <class Par>
KIN_HD bool evaluate(const Par& par, const Ctx& c, const Extra& x, const double* pv, double* e, double& cost) {
  const bool ok = kin::evaluate(par, c, pv, e, cost);
  cost += prior_cost(par, x, pv);
  return ok && finite64(cost);
}

// kin_core.h's linearise at sh.p(), then M += A^-1, g += A^-1 (p - p-), and the held joints taken again from the whole gradient
template <class Par>
KIN_HD void linearise(const Par& par, const Ctx& c, const Extra& x, const double* e) {
  kin::linearise(par, c, e);
  const Shared& sh = c.sh;
  const int N = x.N;
  for (int a = par.lo(); a < par.hi(); ++a)
    if (a < N) {
      double s = sh.g()[a];
      for (int b = 0; b < N; ++b) {
        const double ai = x.Ai()[(size_t)a * N + b];
        sh.M()[a * N + b] += ai;
        s += ai * (sh.p()[b] - x.pm()[b]);
      }
      sh.g()[a] = s;
      bool held = false;
      if (a < c.nfree) {
        const int j = sh.pidx()[a];
        held = (c.pr.q_lo && sh.p()[a] <= (double)c.pr.q_lo[j] && s > 0.0) || (c.pr.q_hi && sh.p()[a] >= (double)c.pr.q_hi[j] && s < 0.0);
      }
      sh.act()[a] = held;
    }
  par.sync();
}

// X = (L L^T)^-1 of the factor in sh.L(), column i by lane i, made symmetric from its lower triangle
template <class Par>
KIN_HD void chol_inverse(const Par& par, const Shared& sh, int N, double* X) {
  for (int i = par.lo(); i < par.hi(); ++i)
    if (i < N) {
      double* col = X + (size_t)i * N;
      for (int r = 0; r < N; ++r) col[r] = r == i ? 1.0 : 0.0;
      kin::chol_apply(sh, N, col);
    }
  par.sync();
  for (int i = par.lo(); i < par.hi(); ++i)
    if (i < N)
      for (int j = i + 1; j < N; ++j) X[(size_t)i * N + j] = X[(size_t)j * N + i];
  par.sync();
}

// the fp32 outputs every path writes.  at_p: q / rot / trans from the evaluation point in sh.q() / sh.pose(), else the inputs bit for bit
template <class Par>
KIN_HD void emit(const Par& par, const Stream& S, const Ctx& c, const Extra& x, bool at_p, int flags, int it, int used, int gated) {
  const Shared& sh = c.sh;
  const Problem& pr = c.pr;
  const uint32_t fm = kin::free_mask(pr.free_q, pr.dof);
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l < pr.dof) pr.q[l] = (at_p && (fm >> l & 1u)) ? (float)sh.q()[l] : S.q_in[l];
    if (l < pr.nkp) {
      if (pr.xyz)
        for (int a = 0; a < 3; ++a) pr.xyz[3 * l + a] = (float)sh.xyz()[3 * l + a];
      if (pr.uv) {
        pr.uv[2 * l] = (float)sh.uv()[2 * l];
        pr.uv[2 * l + 1] = (float)sh.uv()[2 * l + 1];
      }
      if (S.d2) S.d2[l] = (float)x.d2()[l];
    }
    if (l == 0) {
      if (at_p && pr.free_pose) {
        double w[3] = {sh.pose()[0], sh.pose()[1], sh.pose()[2]};
        const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (th > M_PI) {      // kin_core.h's solve_one
          double tn = fmod(th, 2.0 * M_PI);
          if (tn > M_PI) tn -= 2.0 * M_PI;
          for (int a = 0; a < 3; ++a) w[a] *= tn / th;
        }
        if (pr.rot_dim == 3) {
          for (int a = 0; a < 3; ++a) pr.rot[a] = (float)w[a];
        } else {
          double R[3][3];
          kin::rot_aa<double>(w, R);
          for (int a = 0; a < 6; ++a) pr.rot[a] = (float)R[a / 3][a % 3];
        }
        for (int a = 0; a < 3; ++a) pr.trans[a] = (float)sh.pose()[3 + a];
      } else {
        for (int a = 0; a < pr.rot_dim; ++a) pr.rot[a] = S.rot_in[a];
        for (int a = 0; a < 3; ++a) pr.trans[a] = S.trans_in[a];
      }
      if (pr.status) {
        pr.status[0] = flags;
        pr.status[1] = it;
        pr.status[2] = used;
        pr.status[3] = gated;
      }
    }
  }
  par.sync();
}

// xyz_next: FK at pnext (spends sh.pt(), sh.e1() and the evaluation point)
template <class Par>
KIN_HD void emit_next(const Par& par, const Stream& S, const Ctx& c, const double* p, const double* v, bool zero_w) {
  if (!S.xyz_next) return;
  const Shared& sh = c.sh;
  for (int l = par.lo(); l < par.hi(); ++l)
    if (l < c.npar) {
      const bool w = zero_w && l >= c.nfree && l < c.nfree + 3;
      sh.pt()[l] = p[l] + (w ? 0.0 : S.dt * v[l]);
    }
  par.sync();
  double cn;
  kin::evaluate(par, c, sh.pt(), sh.e1(), cn);
  for (int k = par.lo(); k < par.hi(); ++k)
    if (k < c.pr.nkp)
      for (int a = 0; a < 3; ++a) S.xyz_next[3 * k + a] = (float)sh.xyz()[3 * k + a];
  par.sync();
}

template <class Par>
KIN_HD void step_one(const Par& par, const Stream& S, double* buf) {
  Ctx c;
  c.pr = S.pr;
  c.has3d = 0;
  const uint32_t fm = kin::free_mask(c.pr.free_q, c.pr.dof);
  c.nfree = kin::popcount32(fm);
  c.npar = c.nfree + (c.pr.free_pose ? 6 : 0);
  c.nrow = kin::kin_nrow(c.pr.nkp, 0);
  c.sh = kin::carve(buf, c.npar, c.pr.nkp, 0);
  const Extra x{buf + kin::shared_doubles(c.npar, c.pr.nkp, 0), c.npar, c.pr.nkp, c.pr.dof};
  c.pr.q0 = x.q0s();
  const Problem& pr = c.pr;
  const Shared& sh = c.sh;
  const int N = c.npar, nkp = pr.nkp, dof = pr.dof, N2 = 2 * c.npar;
  const double dt = S.dt, dt2 = S.dt * S.dt;
  const double nan = __builtin_nan("");

  // ---- the inputs: the fixed entries of the evaluation point, the usable points, the inputs as a parameter vector -----------------------
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l == 0) {
      double w[3];
      if (pr.rot_dim == 3) {
        for (int a = 0; a < 3; ++a) w[a] = (double)S.rot_in[a];
      } else {
        double r6[6], R[3][3];
        for (int a = 0; a < 6; ++a) r6[a] = (double)S.rot_in[a];
        kin::rot_from_6d(r6, R);
        kin::rot_to_aa(R, w);
      }
      for (int a = 0; a < 3; ++a) {
        sh.pose()[a] = w[a];
        sh.pose()[3 + a] = (double)S.trans_in[a];
      }
    }
    if (l < dof) {
      sh.q()[l] = (double)S.q_in[l];
      x.q0s()[l] = (pr.prior_q && pr.prior_q[l] > 0.f) ? S.q_meas[l] : 0.f;
    }
    if (l < 9) sh.K()[l] = (double)pr.K[l];
    if (l < HRP_FK_MAX_JOINTS) sh.anc()[l] = (int)kin::ancestors(pr.ch, l);
    if (l < nkp) {
      const double w2 = pr.w2d ? (double)pr.w2d[l] : 1.0;
      const bool u2 = w2 > 0.0 && finite64(w2) && finite64((double)pr.pts2d[2 * l]) && finite64((double)pr.pts2d[2 * l + 1]);
      x.su()[l] = u2 ? sqrt(w2) : 0.0;
      x.d2()[l] = nan;
      sh.s3()[l] = 0.0;
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
    if (l < N) x.pin()[l] = l < c.nfree ? sh.q()[sh.pidx()[l]] : sh.pose()[l - c.nfree];
  par.sync();
  int nus = 0;
  for (int k = 0; k < nkp; ++k) nus += x.su()[k] > 0.0;

  // ---- the prior of this frame: the start, or the prediction; a prediction that cannot be used starts again ------------------------------
  bool init = S.valid[0] == 0 || (S.keep && S.keep[0] == 0);
  const int coast_in = S.coast[0];
  bool usable;
  for (;;) {
    for (int l = par.lo(); l < par.hi(); ++l)
      if (l < N) {
        if (init) {
          x.pm()[l] = x.pin()[l];
          x.vm()[l] = 0.0;
          for (int j = 0; j < N; ++j) {
            x.A()[(size_t)l * N + j] = j == l ? S.p0_var[l] : 0.0;
            x.Bm()[(size_t)l * N + j] = 0.0;
            x.Cm()[(size_t)l * N + j] = j == l ? S.p0_var[N + l] : 0.0;
          }
        } else {
          const double* P = S.cov;
          const double qa = S.q_acc[l];
          x.pm()[l] = S.mean[l] + dt * S.mean[N + l];
          x.vm()[l] = S.mean[N + l];
          for (int j = l; j < N; ++j) {
            double a = P[(size_t)l * N2 + j] + dt * (P[(size_t)(N + j) * N2 + l] + P[(size_t)(N + l) * N2 + j]) + dt2 * P[(size_t)(N + l) * N2 + N + j];
            double cc = P[(size_t)(N + l) * N2 + N + j];
            if (j == l) {
              a += qa * (0.25 * dt2 * dt2);
              cc += qa * dt2;
            }
            x.A()[(size_t)l * N + j] = a;
            x.A()[(size_t)j * N + l] = a;
            x.Cm()[(size_t)l * N + j] = cc;
            x.Cm()[(size_t)j * N + l] = cc;
          }
          for (int j = 0; j < N; ++j) {
            const double vv = l <= j ? P[(size_t)(N + l) * N2 + N + j] : P[(size_t)(N + j) * N2 + N + l];
            double b = P[(size_t)(N + l) * N2 + j] + dt * vv;
            if (j == l) b += qa * (0.5 * dt2 * dt);
            x.Bm()[(size_t)l * N + j] = b;
          }
        }
      }
    par.sync();
    for (int l = par.lo(); l < par.hi(); ++l) {
      if (l < N) {
        for (int k = 0; k <= l; ++k) sh.M()[l * N + k] = x.A()[(size_t)l * N + k];
        sh.p()[l] = x.pm()[l];
      }
      if (l < nkp) sh.s2()[l] = x.su()[l];
    }
    par.sync();
    usable = kin::cholesky(par, c, 0.0, false);
    if (usable) chol_inverse(par, sh, N, x.Ai());
    double c0;
    const bool eok = kin::evaluate(par, c, x.pm(), sh.e0(), c0);      // also leaves the evaluation point and xyz / uv for the outputs
    usable = usable && eok;
    if (usable || init) break;
    init = true;
  }
  int flags = init ? HRP_KF_INIT : 0;
  if (!usable) {
    flags |= HRP_KF_BAD_START;
    emit(par, S, c, x, false, flags, 0, 0, 0);
    for (int l = par.lo(); l < par.hi(); ++l) {
      if (l < N) {
        if (S.vel) S.vel[l] = 0.f;
        if (S.cov_p)
          for (int j = 0; j < N; ++j) S.cov_p[(size_t)l * N + j] = 0.f;
      }
      if (l < nkp && S.xyz_next)
        for (int a = 0; a < 3; ++a) S.xyz_next[3 * l + a] = (float)sh.xyz()[3 * l + a];
      if (l == 0) S.valid[0] = 0;
    }
    return;
  }

  // ---- the gate: d2_k of every usable point at p-, from the scaled rows (s H, s r: S~ = s^2 S, the statistic is the same) ----------------
  int ngate = 0;
  if (!init && S.gate > 0.0 && nus > 0) {
    kin::linearise(par, c, sh.e0());
    for (int k = par.lo(); k < par.hi(); ++k)
      if (k < nkp && sh.s2()[k] > 0.0) {
        const double* J0 = sh.J() + 2 * k;
        double s00 = 1.0, s01 = 0.0, s11 = 1.0;
        for (int a = 0; a < N; ++a) {
          double u0 = 0.0, u1 = 0.0;
          for (int b = 0; b < N; ++b) {
            const double ab = x.A()[(size_t)a * N + b];
            u0 += ab * J0[(size_t)b * c.nrow];
            u1 += ab * J0[(size_t)b * c.nrow + 1];
          }
          const double h0 = J0[(size_t)a * c.nrow], h1 = J0[(size_t)a * c.nrow + 1];
          s00 += h0 * u0;
          s01 += h0 * u1;
          s11 += h1 * u1;
        }
        const double r0 = sh.e0()[2 * k], r1 = sh.e0()[2 * k + 1];
        x.d2()[k] = (s11 * r0 * r0 - 2.0 * s01 * r0 * r1 + s00 * r1 * r1) / (s00 * s11 - s01 * s01);
      }
    par.sync();
    for (int k = par.lo(); k < par.hi(); ++k)
      if (k < nkp && x.d2()[k] > S.gate) sh.s2()[k] = 0.0;
    par.sync();
    for (int k = 0; k < nkp; ++k) ngate += x.su()[k] > 0.0 && !(sh.s2()[k] > 0.0);
  }
  const int nused = nus - ngate;

  // ---- the update: kin_core.h's solve_one loop from p-, on the cost with the dense prior ---------------------------------------------------
  int it = 0, converged = 0;
  bool solve = false;
  double *e = sh.e0(), *et = sh.e1();
  if (nused > 0) {
    // the loop starts inside the bounds (a held joint does not move, so a prediction beyond a bound would stay there); the prior's mean
    // stays p- itself
    for (int l = par.lo(); l < par.hi(); ++l)
      if (l < c.nfree) sh.p()[l] = kin::clampq(pr, sh.pidx()[l], x.pm()[l]);
    par.sync();
    int stage = 0;
    double cost = 0.0, lambda = 1e-3, smax = 0.0, ymax = 0.0;
    for (;;) {
      const double* pv = stage == 1 ? sh.pt() : sh.p();
      double cn;
      const bool ok = evaluate(par, c, x, pv, stage == 1 ? et : e, cn);
      if (stage == 2) break;
      bool moved = false, done = false;
      if (stage == 0) {
        cost = cn;
        if (!ok) break;
        solve = true;
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
          if (lambda > 1e10) converged = 1;
        }
        ++it;
        done = converged || it >= kin::KIN_LM_MAX_IT;
      }
      if (moved) linearise(par, c, x, e);
      while (!done && !kin::cholesky(par, c, lambda, true)) {
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
        if (l < N) {
          const double v = sh.p()[l] + sh.step()[l];
          sh.pt()[l] = l < c.nfree ? kin::clampq(pr, sh.pidx()[l], v) : v;
        }
      par.sync();
      smax = ymax = 0.0;
      for (int a = 0; a < N; ++a) {
        smax = fmax(smax, fabs(sh.pt()[a] - sh.p()[a]));
        ymax = fmax(ymax, fabs(sh.p()[a]));
      }
      stage = 1;
    }
  }

  if (!solve) {
    // ---- coast: the prediction (or the start) is the state ---------------------------------------------------------------------------------
    const int base = init ? 0 : coast_in;
    const int cnew = base < 0x7fffffff ? base + 1 : base;
    const bool lost = cnew > S.max_coast;
    flags |= HRP_KF_COASTED | (lost ? HRP_KF_LOST : 0);
    if (nused > 0) {      // the loop's first evaluation refused p-: put the evaluation point and the key-points back
      double c0;
      kin::evaluate(par, c, x.pm(), sh.e0(), c0);
    }
    emit(par, S, c, x, true, flags, 0, 0, ngate);
    for (int l = par.lo(); l < par.hi(); ++l) {
      if (l < N) {
        S.mean[l] = x.pm()[l];
        S.mean[N + l] = x.vm()[l];
        for (int j = 0; j < N; ++j) {
          S.cov[(size_t)l * N2 + j] = x.A()[(size_t)l * N + j];
          S.cov[(size_t)l * N2 + N + j] = x.Bm()[(size_t)j * N + l];
          S.cov[(size_t)(N + l) * N2 + j] = x.Bm()[(size_t)l * N + j];
          S.cov[(size_t)(N + l) * N2 + N + j] = x.Cm()[(size_t)l * N + j];
          if (S.cov_p) S.cov_p[(size_t)l * N + j] = (float)x.A()[(size_t)l * N + j];
        }
        if (S.vel) S.vel[l] = (float)x.vm()[l];
      }
      if (l == 0) {
        S.valid[0] = lost ? 0 : 1;
        S.coast[0] = cnew;
      }
    }
    emit_next(par, S, c, x.pm(), x.vm(), false);
    return;
  }

  if (converged) flags |= HRP_KF_CONVERGED;
  for (int l = 0; l < c.nfree; ++l) {
    const int j = sh.pidx()[l];
    if ((pr.q_lo && sh.p()[l] == (double)pr.q_lo[j]) || (pr.q_hi && sh.p()[l] == (double)pr.q_hi[j])) flags |= HRP_KF_AT_LIMIT;
  }

  // ---- the covariance at p+: sh.M() is J^T W J + diag(w_q) + A^-1 of the last linearisation, which was taken at p+ ------------------------
  if (!kin::cholesky(par, c, 0.0, false)) {
    flags |= HRP_KF_LOST;
    emit(par, S, c, x, true, flags, it, nused, ngate);
    for (int l = par.lo(); l < par.hi(); ++l) {
      if (l < N) {
        if (S.vel) S.vel[l] = 0.f;
        if (S.cov_p)
          for (int j = 0; j < N; ++j) S.cov_p[(size_t)l * N + j] = 0.f;
      }
      if (l < nkp && S.xyz_next)
        for (int a = 0; a < 3; ++a) S.xyz_next[3 * l + a] = (float)sh.xyz()[3 * l + a];
      if (l == 0) S.valid[0] = 0;
    }
    return;
  }
  chol_inverse(par, sh, N, x.Ap());
  for (int i = par.lo(); i < par.hi(); ++i)
    if (i < N)
      for (int j = 0; j < N; ++j) {
        double s = 0.0;
        for (int m = 0; m < N; ++m) s += x.Bm()[(size_t)i * N + m] * x.Ai()[(size_t)m * N + j];
        x.G()[(size_t)i * N + j] = s;
      }
  par.sync();
  for (int i = par.lo(); i < par.hi(); ++i)
    if (i < N) {
      double s = x.vm()[i];
      for (int j = 0; j < N; ++j) {
        s += x.G()[(size_t)i * N + j] * (sh.p()[j] - x.pm()[j]);
        x.A()[(size_t)i * N + j] -= x.Ap()[(size_t)i * N + j];
      }
      x.vp()[i] = s;
    }
  par.sync();
  for (int i = par.lo(); i < par.hi(); ++i)
    if (i < N)
      for (int j = 0; j < N; ++j) {
        double s = 0.0, u = 0.0;
        for (int m = 0; m < N; ++m) {
          s += x.G()[(size_t)i * N + m] * x.Ap()[(size_t)m * N + j];
          u += x.G()[(size_t)i * N + m] * x.A()[(size_t)m * N + j];
        }
        x.Ai()[(size_t)i * N + j] = s;       // P+_vp = G A+
        x.Bm()[(size_t)i * N + j] = u;       // G (A - A+)
      }
  par.sync();
  for (int i = par.lo(); i < par.hi(); ++i)
    if (i < N)
      for (int j = i; j < N; ++j) {
        double s = 0.0;
        for (int m = 0; m < N; ++m) s += x.Bm()[(size_t)i * N + m] * x.G()[(size_t)j * N + m];
        const double v = x.Cm()[(size_t)i * N + j] - s;
        x.Cm()[(size_t)i * N + j] = v;
        x.Cm()[(size_t)j * N + i] = v;
      }
  par.sync();

  // ---- the rotation's wrap, the state, the outputs ---------------------------------------------------------------------------------------
  double wscale = 1.0;
  bool wrapped = false;
  if (pr.free_pose) {
    const double w0 = sh.p()[c.nfree], w1 = sh.p()[c.nfree + 1], w2 = sh.p()[c.nfree + 2];
    const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    if (th > M_PI) {
      double tn = fmod(th, 2.0 * M_PI);
      if (tn > M_PI) tn -= 2.0 * M_PI;
      wscale = tn / th;
      wrapped = true;
      flags |= HRP_KF_REWRAPPED;
    }
  }
  emit(par, S, c, x, true, flags, it, nused, ngate);
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l < N) {
      const bool wl = wrapped && l >= c.nfree && l < c.nfree + 3;
      const double vl = wl ? 0.0 : x.vp()[l];
      S.mean[l] = wl ? wscale * sh.p()[l] : sh.p()[l];
      S.mean[N + l] = vl;
      if (S.vel) S.vel[l] = (float)vl;
      for (int j = 0; j < N; ++j) {
        const bool wj = wrapped && j >= c.nfree && j < c.nfree + 3;
        S.cov[(size_t)l * N2 + j] = x.Ap()[(size_t)l * N + j];
        S.cov[(size_t)l * N2 + N + j] = wj ? 0.0 : x.Ai()[(size_t)j * N + l];
        S.cov[(size_t)(N + l) * N2 + j] = wl ? 0.0 : x.Ai()[(size_t)l * N + j];
        S.cov[(size_t)(N + l) * N2 + N + j] = (wl || wj) ? (l == j ? S.p0_var[N + l] : 0.0) : x.Cm()[(size_t)l * N + j];
        if (S.cov_p) S.cov_p[(size_t)l * N + j] = (float)x.Ap()[(size_t)l * N + j];
      }
    }
    if (l == 0) {
      S.valid[0] = 1;
      S.coast[0] = 0;
    }
  }
  par.sync();
  // FK at p+ + dt v+ (sh.p() keeps w as the loop left it: the same rotation)
  emit_next(par, S, c, sh.p(), x.vp(), wrapped);
}

// the descriptor's pointers narrowed to stream b
KIN_HD Stream stream_of(const hrp_kin_filter_desc& d, int b) {
  const int nkp = d.nkp, dof = d.dof;
  const int n = kin::kin_npar(d.free_q, dof, d.free_pose);
  const size_t bp = d.pose_stride ? (size_t)b : 0;
  Stream s;
  Problem& p = s.pr;
  p.ch = d.chain;
  p.pts2d = d.pts2d + (size_t)b * nkp * 2;
  p.w2d = d.w2d ? d.w2d + (size_t)b * nkp : nullptr;
  p.pts3d = p.w3d = nullptr;
  p.K = d.K + (size_t)b * d.K_stride;
  p.q0 = nullptr;
  p.rot0 = d.rot_in + bp * d.rot_dim;
  p.trans0 = d.trans_in + bp * 3;
  p.q_lo = d.q_lo;
  p.q_hi = d.q_hi;
  p.prior_q = d.w_q;
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
  p.rms = nullptr;
  p.status = d.status ? d.status + (size_t)b * 4 : nullptr;
  p.cov = nullptr;
  s.q_in = d.q_in + (size_t)b * dof;
  s.rot_in = p.rot0;
  s.trans_in = p.trans0;
  s.q_meas = d.q_meas ? d.q_meas + (size_t)b * dof : nullptr;
  s.keep = d.keep ? d.keep + b : nullptr;
  s.q_acc = d.q_acc;
  s.p0_var = d.p0_var;
  s.dt = d.dt;
  s.gate = d.gate_chi2;
  s.max_coast = d.max_coast;
  s.mean = d.mean + (size_t)b * 2 * n;
  s.cov = d.cov + (size_t)b * 4 * n * n;
  s.valid = d.valid + b;
  s.coast = d.coast + b;
  s.vel = d.vel ? d.vel + (size_t)b * n : nullptr;
  s.cov_p = d.cov_p ? d.cov_p + (size_t)b * n * n : nullptr;
  s.xyz_next = d.xyz_next ? d.xyz_next + (size_t)b * nkp * 3 : nullptr;
  s.d2 = d.d2 ? d.d2 + (size_t)b * nkp : nullptr;
  return s;
}

// what hrp_kin_filter_step refuses, as a text (NULL: the descriptor is usable)
KIN_HD const char* refusal(const hrp_kin_filter_desc* d) {
  if (!d) return "null descriptor";
  hrp_kin_desc k = {};
  k.chain = d->chain; k.pts2d = d->pts2d; k.w2d = d->w2d; k.K = d->K; k.K_stride = d->K_stride; k.nkp = d->nkp;
  k.q0 = d->q_in; k.rot0 = d->rot_in; k.trans0 = d->trans_in; k.rot_dim = d->rot_dim; k.pose_stride = d->pose_stride;
  k.free_q = d->free_q; k.free_pose = d->free_pose; k.root = d->root; k.B = d->B; k.dof = d->dof;
  k.q = d->q; k.rot = d->rot; k.trans = d->trans;
  if (const char* why = kin::refusal(&k)) return why;
  if (!(d->dt > 0.0) || !finite64(d->dt)) return "dt must be positive and finite";
  if (d->gate_chi2 != d->gate_chi2) return "gate_chi2 is NaN";
  const int n = kin::kin_npar(d->free_q, d->dof, d->free_pose);
  if (n < 1 || n > MAX_N) return "npar (1..HRP_KIN_FILTER_MAX_N)";
  if (!d->mean || !d->cov || !d->valid || !d->coast) return "null state pointer (mean, cov, valid, coast)";
  if (!d->q_acc || !d->p0_var) return "null q_acc or p0_var";
  if (d->max_coast < 0) return "max_coast < 0";
  if ((d->w_q != nullptr) != (d->q_meas != nullptr)) return "w_q and q_meas go together";
  return nullptr;
}

}  // namespace kinf
}  // namespace hrp
