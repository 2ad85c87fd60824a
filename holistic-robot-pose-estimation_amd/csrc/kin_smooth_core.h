// The kinematic smoother (hrp_kin_smooth, include/hrp.h): a Rauch-Tung-Striebel pass over a recorded history of the kinematic filter's
// posteriors.  Like kin_core.h and kin_filter_core.h it is written once for the kernels of kin_smooth.hip and for a host compiler
// (tests/kinsmooth_host_check.cpp) through a `Par` policy, and it uses kin_core.h as it stands: the key-points of a smoothed frame come
// from kin::evaluate (FK, re-rooting), called, not copied.  Par here gives the lanes this caller executes, [lo(), hi()), their number in
// the workgroup, lanes(), and the barrier: the kernels run lane threadIdx.x of SMOOTH_LANES, the host check runs them one after another.
// A matrix loop is tiled by element (e = lane, lane + lanes(), ...), so the 2n x 2n products of the walk use the whole workgroup and not
// 2n lanes of it; every sum still belongs to one lane and runs in index order, so the bytes do not depend on the number of lanes.
//
//   link_one  one frame t of one stream: is the frame usable, and for t < L-1 the link t -> t+1: P- in closed form from the blocks of
//             P+_t, its Cholesky (right-looking in LDS, thread = element of the trailing block), G = P+_t F^T (P-)^-1 by 2n solves
//             (lane = row of G, stored transposed so that neighbouring lanes touch neighbouring words), the decision
//   walk_one  one stream, t = L-1 .. 0: the mean (a mat-vec), the covariance (two 2n x 2n x 2n products), the outputs
// The Cholesky is a local one of kin::cholesky's shape (right-looking, the roots kept apart from the matrix): kin_core.h's own takes
// its matrix from a kin::Shared carved for npar = 2n, whose Jacobian block alone would be 2n x max(2 nkp, 2n) doubles.
// Of P+_t, P- reads the lower triangles of the (p, p) and (v, v) blocks and the whole (v, p) block; P+_t F^T reads all of it.
#pragma once
#include "kin_core.h"

namespace hrp {
namespace kins {

using kin::Ctx;
using kin::Shared;
using kin::finite64;

constexpr int MAX_N = HRP_KIN_FILTER_MAX_N;
constexpr int SMOOTH_LANES = 256;
enum { LINK_FRAME = 1, LINK_NEXT = 2, LINK_BAD = 4 };      // the scratch's code per frame: usable; linked to t+1; P- or G refused

KIN_HD int npar_of(const hrp_kin_smooth_desc& d) { return kin::kin_npar(d.free_q, d.dof, d.free_pose); }
KIN_HD size_t slot_of(const hrp_kin_smooth_desc& d, int t) { return (size_t)(((int64_t)d.first + t) % d.cap); }
KIN_HD size_t link_doubles(int N) { return 2 * (size_t)N * N + N + 1; }
KIN_HD size_t walk_doubles(int n, int nkp) { return 12 * (size_t)n * n + 4 * (size_t)n + 1 + kin::shared_doubles(n, nkp, 0); }

// entry (i, j), j <= i, of P- = F P F^T + Q for the [2n][2n] matrix P
KIN_HD double pminus(const double* P, const double* q_acc, double dt, int n, int i, int j) {
  const int N = 2 * n, a = i < n ? i : i - n, c = j < n ? j : j - n;
  const int hi = a > c ? a : c, lo = a > c ? c : a;
  const double vv = P[(size_t)(n + hi) * N + n + lo];
  if (i < n) {
    double v = P[(size_t)a * N + c] + dt * (P[(size_t)(n + a) * N + c] + P[(size_t)(n + c) * N + a]) + dt * dt * vv;
    if (a == c) v += q_acc[a] * (0.25 * dt * dt * dt * dt);
    return v;
  }
  if (j < n) {
    double v = P[(size_t)(n + a) * N + c] + dt * vv;
    if (a == c) v += q_acc[a] * (0.5 * dt * dt * dt);
    return v;
  }
  return a == c ? vv + q_acc[a] * (dt * dt) : vv;
}

// valid == 1, and the mean and the covariance's diagonal finite (flag: one shared int)
template <class Par>
KIN_HD bool frame_usable(const Par& par, int* flag, const double* mean, const double* cov, int valid, int N) {
  for (int l = par.lo(); l < par.hi(); ++l)
    if (l == 0) *flag = 0;
  par.sync();
  for (int l = par.lo(); l < par.hi(); ++l)
    for (int e = l; e < 2 * N; e += par.lanes()) {
      const double v = e < N ? mean[e] : cov[(size_t)(e - N) * N + (e - N)];
      if (!finite64(v)) *flag = 1;
    }
  par.sync();
  const bool ok = valid == 1 && !*flag;
  par.sync();
  return ok;
}

template <class Par>
KIN_HD void link_one(const Par& par, const hrp_kin_smooth_desc& d, int t, int b, double* buf) {
  const int n = npar_of(d), N = 2 * n, NN = N * N, B = d.B;
  double* Pm = buf;            // P-, then its factor below the diagonal
  double* Ct = Pm + NN;        // (P+ F^T)^T, then G^T
  double* Ld = Ct + NN;        // the factor's diagonal
  int* flag = (int*)(Ld + N);
  const size_t s0 = slot_of(d, t) * B + b;
  const double* P0 = d.cov + s0 * NN;
  int code = 0;
  const bool ok0 = frame_usable(par, flag, d.mean + s0 * N, P0, d.valid[s0], N);
  if (ok0) code |= LINK_FRAME;
  bool cand = ok0 && t + 1 < d.L;
  size_t s1 = 0;
  if (cand) {
    s1 = slot_of(d, t + 1);
    cand = !(d.flags[s1 * B + b] & (HRP_KF_INIT | HRP_KF_BAD_START | HRP_KF_REWRAPPED));
  }
  if (cand) cand = frame_usable(par, flag, d.mean + (s1 * B + b) * N, d.cov + (s1 * B + b) * NN, d.valid[s1 * B + b], N);
  if (cand) {
    const double dt = d.dt[s1];
    for (int l = par.lo(); l < par.hi(); ++l)
      for (int e = l; e < NN; e += par.lanes()) {
        const int i = e / N, j = e % N;
        if (j <= i) {
          const double v = pminus(P0, d.q_acc, dt, n, i, j);
          Pm[i * N + j] = v;
          Pm[j * N + i] = v;
        }
        Ct[j * N + i] = j < n ? P0[(size_t)i * N + j] + dt * P0[(size_t)i * N + n + j] : P0[(size_t)i * N + j];
      }
    par.sync();
    bool good = true;
    for (int k = 0; k < N; ++k) {
      const double dd = Pm[k * N + k];      // final since step k - 1
      if (!(dd > 0.0) || !finite64(dd)) {
        good = false;
        break;
      }
      const double sd = sqrt(dd);
      for (int l = par.lo(); l < par.hi(); ++l) {
        if (l == k) Ld[k] = sd;
        if (l > k && l < N) Pm[l * N + k] = Pm[l * N + k] / sd;
      }
      par.sync();
      for (int l = par.lo(); l < par.hi(); ++l)
        for (int e = l; e < NN; e += par.lanes()) {
          const int r = e / N, m = e % N;
          if (m > k && m <= r) Pm[r * N + m] -= Pm[r * N + k] * Pm[m * N + k];
        }
      par.sync();
    }
    if (good) {
      for (int i = par.lo(); i < par.hi(); ++i) {
        if (i == 0) *flag = 0;
        if (i < N) {      // row i of G: P- g = (row i of P+ F^T)^T
          for (int r = 0; r < N; ++r) {
            double v = Ct[r * N + i];
            for (int m = 0; m < r; ++m) v -= Pm[r * N + m] * Ct[m * N + i];
            Ct[r * N + i] = v / Ld[r];
          }
          for (int r = N - 1; r >= 0; --r) {
            double v = Ct[r * N + i];
            for (int m = r + 1; m < N; ++m) v -= Pm[m * N + r] * Ct[m * N + i];
            Ct[r * N + i] = v / Ld[r];
          }
        }
      }
      par.sync();
      double* G = d.gain + ((size_t)t * B + b) * NN;
      for (int l = par.lo(); l < par.hi(); ++l)
        for (int e = l; e < NN; e += par.lanes()) {
          const double v = Ct[(e % N) * N + e / N];
          if (!finite64(v)) *flag = 1;
          G[e] = v;
        }
      par.sync();
      good = !*flag;
    }
    code |= good ? LINK_NEXT : LINK_BAD;
  }
  for (int l = par.lo(); l < par.hi(); ++l)
    if (l == 0) d.link[(size_t)t * B + b] = code;
}

template <class Par>
KIN_HD void walk_one(const Par& par, const hrp_kin_smooth_desc& d, int b, double* buf) {
  const int n = npar_of(d), N = 2 * n, NN = N * N, B = d.B, dof = d.dof, nkp = d.nkp;
  double* S = buf;             // P^s of the frame after this one; D = P^s - P-; P^s of this one
  double* Gm = S + NN;
  double* W = Gm + NN;         // G D
  double* xs = W + NN;         // x^s
  double* dv = xs + N;         // x^s_{t+1} - x-
  Ctx c;
  kin::Problem& pr = c.pr;
  pr.ch = d.chain;
  pr.pts2d = pr.w2d = pr.pts3d = pr.w3d = pr.K = pr.q0 = pr.rot0 = pr.trans0 = pr.prior_q = nullptr;
  pr.q_lo = d.q_lo;
  pr.q_hi = d.q_hi;
  pr.nkp = nkp;
  pr.dof = dof;
  pr.rot_dim = d.rot_dim;
  pr.free_pose = d.free_pose;
  pr.root = d.root;
  pr.free_q = d.free_q;
  pr.q = pr.rot = pr.trans = pr.xyz = pr.uv = pr.rms = pr.cov = nullptr;
  pr.status = nullptr;
  c.has3d = 0;
  const uint32_t fm = kin::free_mask(d.free_q, dof);
  c.nfree = kin::popcount32(fm);
  c.npar = n;
  c.nrow = kin::kin_nrow(nkp, 0);
  c.sh = kin::carve(dv + N + 1, n, nkp, 0);
  const Shared& sh = c.sh;
  const int nfree = c.nfree;

  // what kin::evaluate reads besides the parameters: no point is used (s2 = 0), K is the identity (uv is not returned)
  for (int l = par.lo(); l < par.hi(); ++l) {
    if (l == 0 && !d.free_pose) {
      double w[3];
      if (d.rot_dim == 3) {
        for (int a = 0; a < 3; ++a) w[a] = (double)d.rot_fixed[a];
      } else {
        double r6[6], R[3][3];
        for (int a = 0; a < 6; ++a) r6[a] = (double)d.rot_fixed[a];
        kin::rot_from_6d(r6, R);
        kin::rot_to_aa(R, w);
      }
      for (int a = 0; a < 3; ++a) {
        sh.pose()[a] = w[a];
        sh.pose()[3 + a] = (double)d.trans_fixed[a];
      }
    }
    if (l < 9) sh.K()[l] = l % 4 == 0 ? 1.0 : 0.0;
    if (l < HRP_FK_MAX_JOINTS) sh.anc()[l] = (int)kin::ancestors(d.chain, l);
    if (l < nkp) {
      sh.s2()[l] = 0.0;
      sh.s3()[l] = 0.0;
    }
    if (l < nfree) {
      uint32_t m = fm;
      for (int i = 0; i < l; ++i) m &= m - 1;
      int j = 0;
      while (!(m >> j & 1u)) ++j;
      sh.pidx()[l] = j;
    }
  }
  par.sync();

  int count = 0;
  for (int t = d.L - 1; t >= 0; --t) {
    const size_t s0 = slot_of(d, t) * B + b, o = (size_t)t * B + b;
    const double* m0 = d.mean + s0 * N;
    const double* P0 = d.cov + s0 * NN;
    const float* q_in = d.q_in + s0 * dof;
    float* oq = d.q + o * dof;
    float* orot = d.rot + o * d.rot_dim;
    float* otr = d.trans + o * 3;
    float* ovel = d.vel + o * n;
    float* oxyz = d.xyz + o * nkp * 3;
    float* ocp = d.want_cov ? d.cov_p + o * n * n : nullptr;
    double* oms = d.mean_s ? d.mean_s + o * N : nullptr;
    double* ocs = d.want_cov && d.cov_s ? d.cov_s + o * NN : nullptr;
    const int code = d.link[o];
    if (!(code & LINK_FRAME)) {
      for (int l = par.lo(); l < par.hi(); ++l) {
        if (l < dof) oq[l] = 0.f;
        if (l < d.rot_dim) orot[l] = 0.f;
        if (l < 3) otr[l] = 0.f;
        if (l < n) ovel[l] = 0.f;
        if (l < N && oms) oms[l] = 0.0;
        for (int e = l; e < 3 * nkp; e += par.lanes()) oxyz[e] = 0.f;
        if (ocp)
          for (int e = l; e < n * n; e += par.lanes()) ocp[e] = 0.f;
        if (ocs)
          for (int e = l; e < NN; e += par.lanes()) ocs[e] = 0.0;
        if (l == 0) {
          d.status[2 * o] = HRP_KS_INVALID;
          d.status[2 * o + 1] = 0;
        }
      }
      count = 0;
      continue;
    }
    int flags;
    if (code & LINK_NEXT) {
      const double dt = d.dt[slot_of(d, t + 1)];
      const double* G = d.gain + o * NN;
      for (int l = par.lo(); l < par.hi(); ++l) {
        for (int e = l; e < NN; e += par.lanes()) Gm[e] = G[e];
        if (l < N) dv[l] = xs[l] - (l < n ? m0[l] + dt * m0[n + l] : m0[l]);
      }
      par.sync();
      for (int i = par.lo(); i < par.hi(); ++i)
        if (i < N) {
          double s = 0.0;
          for (int j = 0; j < N; ++j) s += Gm[i * N + j] * dv[j];
          xs[i] = m0[i] + s;
        }
      if (d.want_cov) {
        for (int l = par.lo(); l < par.hi(); ++l)
          for (int e = l; e < NN; e += par.lanes()) {
            const int i = e / N, j = e % N;
            if (j <= i) {
              const double v = S[i * N + j] - pminus(P0, d.q_acc, dt, n, i, j);
              S[i * N + j] = v;
              S[j * N + i] = v;
            }
          }
        par.sync();
        for (int l = par.lo(); l < par.hi(); ++l)
          for (int e = l; e < NN; e += par.lanes()) {
            const int i = e / N, j = e % N;
            double s = 0.0;
            for (int k = 0; k < N; ++k) s += Gm[i * N + k] * S[k * N + j];
            W[e] = s;
          }
        par.sync();
        for (int l = par.lo(); l < par.hi(); ++l)
          for (int e = l; e < NN; e += par.lanes()) {
            const int i = e / N, j = e % N;
            if (j <= i) {
              double s = 0.0;
              for (int k = 0; k < N; ++k) s += W[i * N + k] * Gm[j * N + k];
              const double v = P0[(size_t)i * N + j] + s;
              S[i * N + j] = v;
              S[j * N + i] = v;
            }
          }
      }
      par.sync();
      count = count < 0x7fffffff ? count + 1 : count;
      flags = HRP_KS_SMOOTHED;
    } else {
      for (int l = par.lo(); l < par.hi(); ++l) {
        if (l < N) xs[l] = m0[l];
        if (d.want_cov)
          for (int e = l; e < NN; e += par.lanes()) S[e] = P0[e];
      }
      par.sync();
      count = 0;
      flags = HRP_KS_TAIL | ((code & LINK_BAD) ? HRP_KS_BAD_LINK : 0);
    }

    // ---- the outputs: the joints clamped, FK at what is returned -------------------------------------------------------------------------
    for (int l = par.lo(); l < par.hi(); ++l) {
      if (l < dof) sh.q()[l] = (double)q_in[l];
      if (l < n) sh.pt()[l] = l < nfree ? kin::clampq(pr, sh.pidx()[l], xs[l]) : xs[l];
    }
    par.sync();
    for (int l = 0; l < nfree; ++l)
      if (sh.pt()[l] != xs[l]) flags |= HRP_KS_CLAMPED;
    pr.q0 = q_in;
    double cn;
    kin::evaluate(par, c, sh.pt(), sh.e0(), cn);
    for (int l = par.lo(); l < par.hi(); ++l) {
      if (l < dof) oq[l] = (fm >> l & 1u) ? (float)sh.q()[l] : q_in[l];
      if (l < n) ovel[l] = (float)xs[n + l];
      if (l < N && oms) oms[l] = xs[l];
      for (int e = l; e < 3 * nkp; e += par.lanes()) oxyz[e] = (float)sh.xyz()[e];
      if (ocp)
        for (int e = l; e < n * n; e += par.lanes()) ocp[e] = (float)S[(e / n) * N + e % n];
      if (ocs)
        for (int e = l; e < NN; e += par.lanes()) ocs[e] = S[e];
      if (l == 0) {
        if (d.free_pose) {
          double w[3] = {sh.pose()[0], sh.pose()[1], sh.pose()[2]};
          const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
          if (th > M_PI) {      // kin_filter_core.h's emit
            double tn = fmod(th, 2.0 * M_PI);
            if (tn > M_PI) tn -= 2.0 * M_PI;
            for (int a = 0; a < 3; ++a) w[a] *= tn / th;
          }
          if (d.rot_dim == 3) {
            for (int a = 0; a < 3; ++a) orot[a] = (float)w[a];
          } else {
            double R[3][3];
            kin::rot_aa<double>(w, R);
            for (int a = 0; a < 6; ++a) orot[a] = (float)R[a / 3][a % 3];
          }
          for (int a = 0; a < 3; ++a) otr[a] = (float)sh.pose()[3 + a];
        } else {
          for (int a = 0; a < d.rot_dim; ++a) orot[a] = d.rot_fixed[a];
          for (int a = 0; a < 3; ++a) otr[a] = d.trans_fixed[a];
        }
        d.status[2 * o] = flags;
        d.status[2 * o + 1] = count;
      }
    }
    par.sync();
  }
}

// what hrp_kin_smooth refuses, as a text (NULL: the descriptor is usable)
KIN_HD const char* refusal(const hrp_kin_smooth_desc* d) {
  if (!d) return "null descriptor";
  if (!d->chain || !d->mean || !d->cov || !d->valid || !d->flags || !d->dt || !d->q_acc) return "null pointer (chain, mean, cov, valid, flags, dt, q_acc)";
  if (!d->gain || !d->link) return "null scratch pointer (gain, link)";
  if ((d->dof > 0 && !d->q) || !d->rot || !d->trans || !d->vel || !d->xyz || !d->status) return "null output pointer (q, rot, trans, vel, xyz, status)";
  if (d->want_cov && !d->cov_p) return "want_cov without cov_p";
  if (d->B < 1) return "B < 1";
  if (d->cap < 1) return "cap < 1";
  if (d->L < 1) return "L < 1";
  if (d->L > d->cap) return "L > cap";
  if (d->first < 0 || d->first >= d->cap) return "first outside 0 .. cap - 1";
  if (d->dof < 0 || d->dof > HRP_FK_MAX_JOINTS) return "dof (0..HRP_FK_MAX_JOINTS)";
  if (d->dof > 0 && !d->q_in) return "null q_in";
  if (d->nkp < 1 || d->nkp > HRP_FK_MAX_KP) return "nkp (1..HRP_FK_MAX_KP)";
  if (d->free_pose != 0 && d->free_pose != 1) return "free_pose is 0 or 1";
  if (d->dof < 32 && (d->free_q >> d->dof)) return "a free_q bit at or above dof";
  if (d->root < 0 || d->root >= d->nkp) return "root outside 0 .. nkp - 1";
  if (d->rot_dim != 3 && d->rot_dim != 6) return "rot_dim is 3 or 6";
  if (!d->free_pose && (!d->rot_fixed || !d->trans_fixed)) return "free_pose == 0 needs rot_fixed and trans_fixed";
  const int n = npar_of(*d);
  if (n < 1 || n > MAX_N) return "npar (1..HRP_KIN_FILTER_MAX_N)";
  return nullptr;
}

KIN_HD const char* push_refusal(const hrp_kin_history_desc* d) {
  if (!d) return "null descriptor";
  if (!d->mean || !d->cov || !d->valid || !d->status) return "null state pointer (mean, cov, valid, status)";
  if (!d->h_mean || !d->h_cov || !d->h_valid || !d->h_flags || !d->h_dt) return "null ring pointer";
  if (d->B < 1) return "B < 1";
  if (d->n < 1 || d->n > MAX_N) return "n (1..HRP_KIN_FILTER_MAX_N)";
  if (d->dof < 0 || d->dof > HRP_FK_MAX_JOINTS) return "dof (0..HRP_FK_MAX_JOINTS)";
  if (d->dof > 0 && (!d->q_in || !d->h_q_in)) return "null q_in";
  if (d->cap < 1) return "cap < 1";
  if (d->slot < 0 || d->slot >= d->cap) return "slot outside 0 .. cap - 1";
  if (!(d->dt > 0.0) || !finite64(d->dt)) return "dt must be positive and finite";
  return nullptr;
}

}  // namespace kins
}  // namespace hrp
