"""Generate tests/golden/golden_kinfit.npz: cases for the kinematic refit (hrp_kin_solve) with their float64 optima.

Run by hand on the CPU:  ``python tests/golden/gen_golden_kinfit.py``  (numpy, scipy 1.15; the chains come from URDFRobot on the URDFs
under holistic-robot-pose-estimation_amd/assets).  The oracle is tests/kinfit_oracle.py: float64 numpy FK from the chain tables and
``scipy.optimize.least_squares`` on the cost of include/hrp.h.

Per robot (panda, kuka, baxter), K = [[600, 0, 320], [0, 600, 240], [0, 0, 1]], the robot about 1.5 m away, a seeded configuration inside
the joint bounds, the start 0.15 rad off on the observable joints (and 0.05 rad / 0.03 m off on a free pose):
  qonly         pose fixed, exact projections                    qonly_noise   the same with +-1 px uniform noise
  both_prior    pose and observable joints free, prior_q = 1 on every free joint, +-1 px noise
  both_q1fixed  pose free, no prior, joint 1 (column 0) not free, +-1 px noise
  with3d        both_prior plus camera-frame 3-D targets (+-2 mm noise) with w3d = 1e4
  limit         qonly_noise with the generating value of one joint 0.1 rad outside its bound: the bounded optimum sits on it
  weights       qonly_noise with per-point weights, two of them 0, one of those points NaN
  root3         (panda only) both_prior with root = 3
Inputs are stored in float32 and the optimum p* (free joints ascending, then w, t) is that of the stored values.  Every case carries the
joint bounds as q_lo / q_hi.  Asserted per case - a draw that fails is redrawn with the next seed, the conditions never move:
  * scipy from a second start, and from inputs moved by half an fp32 ulp, ends within 1e-6 of p* (a tenth of the gate);
  * the LM loop of hrp_kin_solve restated in numpy (kinfit_oracle.Problem.lm) ends within 1e-6 of p* in at most 100 of its 200 trials,
    converged, with the flags stored as <c>_flags;
  * every used point has positive depth at p*; p* lies inside the bounds, except in ``limit`` where exactly one joint is ON its bound
    (found with bounds by scipy's trf, then the joint is set on the bound and the rest solved again; the gradient there points across it);
  * the largest entry of the weighted Jacobian at p* is below 1000 px per unit (stored as <c>_maxJ; the largest over the file is printed).
Keys per case <c> (kinfit_oracle.encode_case / load_fixture): <c>_in float32, the inputs laid end to end (pts2d, [w2d], [pts3d, w3d], q0,
rot0, trans0, lo, hi, [prior]); <c>_meta int32 (robot, nkp, dof, rot_dim, free_pose, root, free bits, present bits, flags, trials, seed);
<c>_ref float64 (rms at p*, maxJ, p*).  ``K`` is shared and ``cases`` lists the names."""
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
import kinfit_oracle as ko  # noqa: E402
from hrpe_amd.lib.dataset.const import JOINT_BOUNDS  # noqa: E402
from hrpe_amd.lib.utils.kinfit import observable_joints  # noqa: E402
from hrpe_amd.lib.utils.urdf_robot import URDFRobot  # noqa: E402

K = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]], dtype=np.float32)
KINDS = ["qonly", "qonly_noise", "both_prior", "both_q1fixed", "with3d", "limit", "weights"]
TOL = dict(xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)


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
    return p


def draw(robot, kind, seed):
    name = robot.robot_type
    rng = np.random.default_rng(seed)
    ch = robot.chain
    dof, nkp = int(ch.dof), int(ch.nkp)
    lim = np.array(JOINT_BOUNDS[name], dtype=np.float64)
    lo, hi = f32(lim[:, 0]), f32(lim[:, 1])
    obs = observable_joints(robot)
    q = lim[:, 0] + (0.2 + 0.6 * rng.random(dof)) * (lim[:, 1] - lim[:, 0])
    pose = np.array([1.2, -1.0, 0.8, 0.05, -0.1, 1.5]) + 0.1 * rng.standard_normal(6)
    root = 3 if kind == "root3" else 0
    on = None
    if kind == "limit":
        on = int(rng.choice(np.flatnonzero(obs)[1:5]))
        q[on] = lim[on, 1] + 0.1
    tab = ko.tables(ch)
    X = ko.keypoints(tab, q, ko.rodrigues(pose[:3]), pose[3:], root)
    x = ko.project(K, X)
    if kind != "qonly":
        x = x + rng.uniform(-1, 1, x.shape)
    free_pose = kind in ("both_prior", "both_q1fixed", "with3d", "root3")
    free = obs.copy()
    if kind == "both_q1fixed":
        free[0] = False
    q0 = np.clip(q + 0.15 * rng.standard_normal(dof) * obs, lim[:, 0] + 0.01, lim[:, 1] - 0.01)
    if not free_pose or kind == "both_q1fixed":
        q0 = np.where(free, q0, np.clip(q, lim[:, 0], lim[:, 1]))       # what is not solved is known
    pose0 = pose + (np.r_[0.05 * rng.standard_normal(3), 0.03 * rng.standard_normal(3)] if free_pose else 0.0)
    case = dict(chain=ch, robot=name, pts2d=f32(x), K=K, q0=f32(q0), rot0=f32(pose0[:3]), trans0=f32(pose0[3:]), lo=lo, hi=hi,
                free=free, free_pose=free_pose, root=root)
    if kind in ("both_prior", "with3d", "root3"):
        case["prior"] = f32(np.where(free, 1.0, 0.0))
    if kind == "with3d":
        case["pts3d"], case["w3d"] = f32(X + rng.uniform(-0.002, 0.002, X.shape)), f32(np.full(nkp, 1e4))
    if kind == "weights":
        w = 0.5 + rng.random(nkp)
        off = rng.choice(nkp, 2, replace=False)
        w[off] = 0.0
        case["w2d"] = f32(w)
        case["pts2d"][off[0]] = np.nan
    return case, on


def conditions(case, on):
    P = ko.Problem(case)
    if on is None:
        p = scipy_optimum(P, P.p0)
        inside = (p > P.plo).all() and (p < P.phi).all()
        if not inside:
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
        g = P.jacobian(p).T @ P.residuals(p)[0]
        outward = g[i] < 0 if fixed[i] == P.phi[i] else g[i] > 0
        others = np.delete(np.arange(P.npar), i)
        if not outward or not ((p[others] > P.plo[others]).all() and (p[others] < P.phi[others]).all()):
            return None, "the bounded optimum is not on exactly one bound"
        if int(np.flatnonzero(P.free)[i]) != on:
            return None, "another joint than the planted one is on its bound"
    rng = np.random.default_rng(7)
    p2 = scipy_optimum(P, p + 0.02 * rng.standard_normal(P.npar), fixed)
    if np.abs(p2 - p).max() > 1e-6:
        return None, f"a second start ends {np.abs(p2 - p).max():.2e} away"
    moved = dict(case)
    for k in ("pts2d", "pts3d"):
        if case.get(k) is not None:
            a = case[k].astype(np.float64)
            moved[k] = a + 0.5 * np.spacing(np.abs(case[k])).astype(np.float64) * rng.choice([-1.0, 1.0], a.shape)
    p3 = scipy_optimum(ko.Problem(moved), p, fixed)
    if np.abs(p3 - p).max() > 1e-6:
        return None, f"inputs moved by half an ulp end {np.abs(p3 - p).max():.2e} away"
    pl, flags, it = P.lm()
    if np.abs(pl - p).max() > 1e-6 or it > 100 or not flags & ko.CONVERGED:
        return None, f"the restated LM ends {np.abs(pl - p).max():.2e} away after {it} trials, flags {flags}"
    if bool(flags & ko.AT_LIMIT) != (on is not None):
        return None, f"flags {flags}"
    if not (P.points(p)[:, 2] > 0).all():
        return None, "a point behind the camera"
    maxJ = float(np.abs(P.jacobian(p)).max())
    if maxJ >= 1000:
        return None, f"Jacobian entry {maxJ}"
    return dict(p_star=p, rms=P.rms(p), flags=np.int32(flags), trials=np.int32(it), maxJ=maxJ), None


def main():
    out, names, worst = {}, [], 0.0
    for ri, name in enumerate(("panda", "kuka", "baxter")):
        robot = URDFRobot(name)
        for ki, kind in enumerate(KINDS + (["root3"] if name == "panda" else [])):
            for seed in range(1000 * ri + 100 * ki, 1000 * ri + 100 * ki + 40):
                case, on = draw(robot, kind, seed)
                got, why = conditions(case, on)
                if got is not None:
                    break
                print(f"  {name}_{kind} seed {seed}: {why}")
            else:
                raise SystemExit(f"{name}_{kind}: no seed met the conditions")
            c = f"{name}_{kind}"
            names.append(c)
            worst = max(worst, got["maxJ"])
            print(f"{c}: seed {seed}, npar {len(got['p_star'])}, rms {got['rms']:.3e}, LM trials {got['trials']}, flags {got['flags']}, max |J| {got['maxJ']:.1f}")
            out.update(ko.encode_case(c, case, dict(got, seed=seed)))
    out["K"] = K
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "golden_kinfit.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(names)} cases, largest Jacobian entry {worst:.1f}")


if __name__ == "__main__":
    main()
