"""Generate tests/golden/golden_kinviews.npz: cases for the multi-view kinematic refit (hrp_kin_solve_views) with their float64 optima.

Run by hand on the CPU:  ``python tests/golden/gen_golden_kinviews.py``  (numpy, scipy; the chains come from URDFRobot on the URDFs
under holistic-robot-pose-estimation_amd/assets).  The oracle is tests/kinviews_oracle.py: float64 numpy FK from the chain tables and
``scipy.optimize.least_squares`` on the cost of include/hrp.h, polished by Gauss-Newton steps with the complex-step Jacobian.

The cameras stand at kinviews_oracle.CAMERAS in the base frame and look at (0, 0, 0.4); K = [[600, 0, 320], [0, 600, 240], [0, 0, 1]] for
every view; a case of V views uses the first V cameras.  Per robot (panda, kuka, baxter): a seeded configuration inside the joint bounds,
+-1 px uniform noise on every projection, the start 0.15 rad off on the observable joints, which are the free ones:
  v2, v3, v4     V views
  occluded       3 views: view 1 loses half its key-points by weight 0, view 0 has one key-point NaN
  occluded_view  the same, and view 2 is NaN altogether
  weights        3 views, per-point weights 0.25 * 16^u, u uniform in [0, 1)
  limit          2 views, the generating value of one of the observable joints 1 .. 4 0.1 rad beyond its upper bound
  prior          2 views, prior_q = 1 on every free joint
  shared_vs_per_sample   2 views; the tests lay the same data out with shared and with per-sample K and poses
Inputs are stored in float32 and the optimum p* (free joints ascending) is that of the stored values.  Every case carries the joint bounds
as q_lo / q_hi.  Asserted per case - a draw that fails is redrawn with the next seed, the conditions never move:
  * scipy from a second start, and from inputs moved by half an fp32 ulp, ends within 1e-6 of p* (a tenth of the gate);
  * the LM loop of hrp_kin_solve_views restated in numpy (kinviews_oracle.Problem.lm) ends within 1e-6 of p* in at most 100 of its
    HRP_KIN_MAX_IT = 200 trials, converged, with the flags stored in <c>_meta;
  * every used point has positive depth in its view at p*; p* lies inside the bounds, except in ``limit`` where exactly the planted joint
    is ON its bound (found with bounds by scipy's trf, then the joint is set on the bound and the rest solved again; the gradient there
    points across it);
  * the gradient of C / 2 at p*, over the joints that are not on a bound, is below GRAD_TOL = 1e-5 px^2 / rad in norm.  With J^T J of
    1e3 .. 1e6 px^2 / rad^2 that is a distance of 1e-8 rad or less to the stationary point, a thousandth of the gate.
Keys per case <c> (kinviews_oracle.encode_case / load_fixture): <c>_in float32, the inputs laid end to end (pts2d, [w2d], q0, lo, hi,
[prior]); <c>_meta int32 (robot, nkp, dof, V, free bits, present bits, flags, trials, seed); <c>_ref float64 (rms at p*, the gradient
norm, the covariance figure of the oracle alone - numpy at p* rounded to fp32 against numpy at p*, relative to sqrt(cov_ii cov_jj), 0 for
``limit`` whose covariance is not written -, rms_view [V], p*).  ``K``, ``poses`` [4, 6] fp32, ``grad_tol`` and ``cases`` are shared.

experiment_<robot> = (one view, two views): the RMS over SEEDS of the largest joint error of kinviews_oracle.Problem.lm, joint limits
on, from +-1 px noise and a start 0.15 rad off, with view 0 alone and with views 0 + 1.  Asserted: two views give at most half the error
of one.  (Without limits scipy measured ratios of 0.11, 0.10 and 0.02 over 8 seeds; the limits help one view most, and here the ratios
are 0.40, 0.40 and 0.42.  The RMS is carried by the few draws in which a distal joint is barely observable from either camera: over
the first 8 of these seeds alone the ratios are 0.19, 0.32 and 0.59, Baxter's from one draw with 0.30 rad on its joint 9 in both
runs, which is why the sample is 32 seeds and not 8.)"""
import os
import sys

import numpy as np
from scipy.optimize import least_squares

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hrpe_amd  # noqa: E402,F401
import kinviews_oracle as kv  # noqa: E402
from hrpe_amd.lib.dataset.const import JOINT_BOUNDS  # noqa: E402
from hrpe_amd.lib.utils.kinfit import observable_joints  # noqa: E402
from hrpe_amd.lib.utils.urdf_robot import URDFRobot  # noqa: E402

K = kv.K0.astype(np.float32)
POSES = np.stack([kv.look_at(c) for c in kv.CAMERAS]).astype(np.float32)
VIEWS = dict(v2=2, v3=3, v4=4, occluded=3, occluded_view=3, weights=3, limit=2, prior=2, shared_vs_per_sample=2)
TOL = dict(xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
GRAD_TOL = 1e-5
SEEDS = range(5000, 5032)


def f32(v):
    return np.asarray(v, dtype=np.float32)


def scipy_optimum(P, start, fixed=None):
    """least_squares (lm) over the parameters that are not fixed at a value."""
    free = np.ones(P.npar, bool)
    base = np.asarray(start, dtype=np.float64).copy()
    if fixed:
        for i, v in fixed.items():
            free[i], base[i] = False, v

    def fun(z):
        p = base.copy()
        p[free] = z
        return P.residuals(p)[0]
    r = least_squares(fun, base[free], method="lm", **TOL)
    p = base.copy()
    p[free] = r.x
    # scipy differences the residuals for its Jacobian and stops at a gradient of 1e-5 .. 1e-4; Gauss-Newton steps with the
    # complex-step Jacobian, which is exact, take the stationary point to rounding
    for _ in range(20):
        J = P.jacobian(p)[:, free]
        g = J.T @ P.residuals(p)[0]
        if np.linalg.norm(g) < 1e-9:
            break
        p[free] -= np.linalg.solve(J.T @ J, g)
    return p


def draw(robot, kind, seed, V=None):
    """(case, planted joint or None, the generating joints)."""
    name = robot.robot_type
    rng = np.random.default_rng(seed)
    ch = robot.chain
    dof, nkp = int(ch.dof), int(ch.nkp)
    V = VIEWS[kind] if V is None else V
    lim = np.array(JOINT_BOUNDS[name], dtype=np.float64)
    obs = observable_joints(robot)
    q = lim[:, 0] + (0.2 + 0.6 * rng.random(dof)) * (lim[:, 1] - lim[:, 0])
    on = None
    if kind == "limit":
        on = int(rng.choice(np.flatnonzero(obs)[1:5]))
        q[on] = lim[on, 1] + 0.1
    q0 = np.clip(q + 0.15 * rng.standard_normal(dof) * obs, lim[:, 0] + 0.01, lim[:, 1] - 0.01)
    q0 = np.where(obs, q0, np.clip(q, lim[:, 0], lim[:, 1]))       # what is not solved is known
    case = dict(chain=ch, robot=name, K=np.repeat(K[None], V, 0), poses=POSES[:V].copy(), q0=f32(q0), lo=f32(lim[:, 0]), hi=f32(lim[:, 1]),
                free=obs.copy(), pts2d=np.zeros((V, nkp, 2), np.float32))
    x = kv.Problem(case).reprojection(q[obs])[0]
    x = f32(x + rng.uniform(-1, 1, x.shape))
    if kind in ("occluded", "occluded_view"):
        w = np.ones((V, nkp))
        w[1, rng.choice(nkp, nkp // 2, replace=False)] = 0.0
        x[0, int(rng.integers(nkp))] = np.nan
        if kind == "occluded_view":
            x[2] = np.nan
        case["w2d"] = f32(w)
    if kind == "weights":
        case["w2d"] = f32(0.25 * 16.0 ** rng.random((V, nkp)))
    if kind == "prior":
        case["prior"] = f32(np.where(obs, 1.0, 0.0))
    case["pts2d"] = x
    return case, on, q


def conditions(case, on):
    P = kv.Problem(case)
    if on is None:
        p = scipy_optimum(P, P.p0)
        if not ((p > P.plo).all() and (p < P.phi).all()):
            return None, "optimum outside the bounds"
        fixed = None
    else:
        r = least_squares(lambda z: P.residuals(z)[0], np.clip(P.p0, P.plo + 1e-6, P.phi - 1e-6), bounds=(P.plo, P.phi), method="trf", **TOL)
        near = np.flatnonzero((r.x - P.plo < 1e-6) | (P.phi - r.x < 1e-6))
        if len(near) != 1:
            return None, f"{len(near)} joints near a bound"
        i = int(near[0])
        fixed = {i: P.phi[i] if P.phi[i] - r.x[i] < 1e-6 else P.plo[i]}
        p = scipy_optimum(P, r.x, fixed)
        g = P.gradient(p)
        outward = g[i] < 0 if fixed[i] == P.phi[i] else g[i] > 0
        others = np.delete(np.arange(P.npar), i)
        if not outward or not ((p[others] > P.plo[others]).all() and (p[others] < P.phi[others]).all()):
            return None, "the bounded optimum is not on exactly one bound"
        if int(P.idx[i]) != on:
            return None, "another joint than the planted one is on its bound"
    rng = np.random.default_rng(7)
    p2 = scipy_optimum(P, p + 0.02 * rng.standard_normal(P.npar), fixed)
    if np.abs(p2 - p).max() > 1e-6:
        return None, f"a second start ends {np.abs(p2 - p).max():.2e} away"
    moved = dict(case)
    a = case["pts2d"].astype(np.float64)
    moved["pts2d"] = a + 0.5 * np.spacing(np.abs(case["pts2d"])).astype(np.float64) * rng.choice([-1.0, 1.0], a.shape)
    p3 = scipy_optimum(kv.Problem(moved), p, fixed)
    if np.abs(p3 - p).max() > 1e-6:
        return None, f"inputs moved by half an ulp end {np.abs(p3 - p).max():.2e} away"
    pl, flags, it = P.lm()
    if np.abs(pl - p).max() > 1e-6 or it > 100 or not flags & kv.CONVERGED:
        return None, f"the restated LM ends {np.abs(pl - p).max():.2e} away after {it} trials, flags {flags}"
    if bool(flags & kv.AT_LIMIT) != (on is not None):
        return None, f"flags {flags}"
    on_bound = (p == P.plo) | (p == P.phi)
    if int(on_bound.sum()) != (0 if on is None else 1):
        return None, f"{int(on_bound.sum())} joints on a bound"
    if not (P.points(p)[:, :, 2][P.u2] > 0).all():
        return None, "a used point behind its camera"
    grad = float(np.linalg.norm(P.gradient(p)[~on_bound]))
    if grad >= GRAD_TOL:
        return None, f"gradient {grad:.2e}"
    sv = float(np.linalg.svd(P.jacobian(p), compute_uv=False).min())
    rel = lambda a, b: float((np.abs(a - b) / np.sqrt(np.outer(np.diag(b), np.diag(b)))).max())      # noqa: E731
    own = 0.0 if on is not None else rel(P.covariance(p.astype(np.float32).astype(np.float64)), P.covariance(p))
    return dict(p_star=p, rms=P.rms(p), rms_view=P.rms_view(p), flags=np.int32(flags), trials=np.int32(it), grad=grad, cov_own=own, sv=sv,
                depth=float(P.points(p)[:, :, 2][P.u2].min())), None


def experiment(robot):
    """RMS over SEEDS of the largest joint error with view 0 alone and with views 0 + 1, joint limits on."""
    err = []
    for seed in SEEDS:
        case, _, q = draw(robot, "v2", seed)
        one = dict(case, pts2d=case["pts2d"][:1], K=case["K"][:1], poses=case["poses"][:1])
        e = []
        for c in (one, case):
            P = kv.Problem(c)
            p, _, _ = P.lm()
            e.append(np.abs(p - q[P.idx]).max())
        err.append(e)
    return np.sqrt((np.array(err) ** 2).mean(0))


def main():
    out, names = {}, []
    for ri, name in enumerate(kv.ROBOTS):
        robot = URDFRobot(name)
        for ki, kind in enumerate(kv.KINDS):
            for seed in range(1000 * ri + 100 * ki, 1000 * ri + 100 * ki + 100):
                case, on, _ = draw(robot, kind, seed)
                got, why = conditions(case, on)
                if got is not None:
                    break
                print(f"  {name}_{kind} seed {seed}: {why}")
            else:
                raise SystemExit(f"{name}_{kind}: no seed met the conditions")
            c = f"{name}_{kind}"
            names.append(c)
            print(f"{c}: seed {seed}, V {VIEWS[kind]}, npar {len(got['p_star'])}, rms {got['rms']:.3f}, LM trials {got['trials']}, flags {got['flags']}, "
                  f"gradient {got['grad']:.1e}, smallest singular value {got['sv']:.1f} px/rad, smallest depth {got['depth']:.2f} m, "
                  f"cov alone {got['cov_own']:.1e}")
            out.update(kv.encode_case(c, case, dict(got, seed=seed)))
        e = experiment(robot)
        print(f"{name}: largest joint error, RMS over {len(SEEDS)} seeds: one view {e[0]:.3f} rad, two views {e[1]:.3f} rad, ratio {e[1] / e[0]:.2f}")
        assert e[1] <= 0.5 * e[0], (name, e)
        out[f"experiment_{name}"] = e
    out["K"], out["poses"], out["grad_tol"] = K, POSES, np.float64(GRAD_TOL)
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "golden_kinviews.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(names)} cases")


if __name__ == "__main__":
    main()
