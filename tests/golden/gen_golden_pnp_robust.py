"""Generate tests/golden/golden_pnp_robust.npz: key-points with planted gross outliers for the robust PnP (hrp_pnp_solve_robust).

Run by hand:  ``python tests/golden/gen_golden_pnp_robust.py``  (numpy and scipy only; reads golden_pnp.npz next to it).

Cases, B = 8 each.  3-D points, K and generating poses of ``panda_s0`` (n = 7), ``kuka_s1`` (n = 8) and ``baxter_s1`` (n = 17) come from
golden_pnp.npz; ``cloud24`` has 24 seeded random points in a 0.6 m cube whose centre lies 1-2 m in front of the camera (C(24, 3) = 2024
hypotheses, above the solver's default budget of 1024: the sampled path).  The points are projected with the generating pose, sigma =
0.5 px noise is added, and k points per sample are displaced by 30-100 px in a seeded random direction:
  panda_s0  k = 1 (even samples), 2 (odd samples)     kuka_s1  k = 2     baxter_s1  k = 5     cloud24  k = 8
so every sample keeps at least 5 inliers.  pts2d is stored in float32, and the optima below are those of the stored values.

Expected values, both from ``scipy.optimize.least_squares(method="lm")`` in fp64 on the objective of golden_pnp.npz:
  <c>_P6d      the optimum over the planted inliers, started at the generating pose
  <c>_P6d_all  the optimum over all points, started at <c>_P6d: what a solver without consensus returns
  <c>_mask     the planted inlier mask [B, n] uint8
Asserted for every sample (a seed that fails any of them is skipped, the conditions never move; <c>_seed records the seed used):
  every planted inlier is below 2 px and every planted outlier above 10 px at <c>_P6d, and <c>_P6d_all differs from <c>_P6d by more than
  1e-3 rad or 1e-3 m.
Other keys: <c>_pts2d [B,n,2] f32, <c>_pts3d [B,n,3] f32, <c>_K [3,3] f32, cases."""
import os

import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
SIGMA, B = 0.5, 8
CASES = [("panda_s0", "panda_s0", (1, 2), 101), ("kuka_s1", "kuka_s1", (2, 2), 102), ("baxter_s1", "baxter_s1", (5, 5), 103),
         ("cloud24", None, (8, 8), 104)]


def project(P6d, X, K):
    R = Rotation.from_rotvec(P6d[:3]).as_matrix()
    p = (X @ R.T + P6d[3:]) @ K.T
    return p[:, :2] / p[:, 2:3]


def solve_lm(x, X, K, init):
    return least_squares(lambda p: (project(p, X, K) - x).ravel(), init, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                         max_nfev=20000).x


def pose_gap(a, b):
    D = Rotation.from_rotvec(a[:3]).inv() * Rotation.from_rotvec(b[:3])
    return np.linalg.norm(D.as_rotvec()), np.abs(a[3:] - b[3:]).max()


def cloud(g):
    X = g.uniform(-0.3, 0.3, (B, 24, 3))
    P = np.zeros((B, 6))
    for i in range(B):
        ax = g.normal(size=3)
        w = ax / np.linalg.norm(ax) * g.uniform(0.1, 3.0)
        d = g.uniform(1.0, 2.0)
        P[i] = np.concatenate([w, [g.uniform(-0.15, 0.15) * d, g.uniform(-0.1, 0.1) * d, d]])
    return X.astype(np.float32).astype(np.float64), P


def try_case(gold, src, ks, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    K = gold["panda_s0_K"].astype(np.float64) if src is None else gold[f"{src}_K"].astype(np.float64)
    if src is None:
        X, P_true = cloud(g)
    else:
        X, P_true = gold[f"{src}_pts3d"].astype(np.float64), gold[f"{src}_P6d_true"]
    n = X.shape[1]
    pts2d, mask = np.zeros((B, n, 2), np.float32), np.ones((B, n), np.uint8)
    P_in, P_all = np.zeros((B, 6)), np.zeros((B, 6))
    for i in range(B):
        x = project(P_true[i], X[i], K) + g.normal(0, SIGMA, (n, 2))
        k = ks[i % 2]
        out = g.choice(n, size=k, replace=False)
        ang, r = g.uniform(0, 2 * np.pi, k), g.uniform(30, 100, k)
        x[out] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
        mask[i, out] = 0
        pts2d[i] = x.astype(np.float32)
        x = pts2d[i].astype(np.float64)
        m = mask[i].astype(bool)
        P_in[i] = solve_lm(x[m], X[i][m], K, P_true[i])
        P_all[i] = solve_lm(x, X[i], K, P_in[i])
        e = np.sqrt(((project(P_in[i], X[i], K) - x) ** 2).sum(1))
        dr, dt = pose_gap(P_in[i], P_all[i])
        if m.sum() < 5 or not (e[m] < 2).all() or not (e[~m] > 10).all() or not (dr > 1e-3 or dt > 1e-3):
            return None
    return {"pts2d": pts2d, "pts3d": X.astype(np.float32), "K": K.astype(np.float32), "P6d": P_in, "P6d_all": P_all, "mask": mask,
            "seed": np.int32(seed)}


def main():
    gold = np.load(os.path.join(HERE, "golden_pnp.npz"))
    out = {}
    for name, src, ks, seed in CASES:
        for s in range(seed, seed + 100000, 1000):
            got = try_case(gold, src, ks, s)
            if got is not None:
                break
        else:
            raise SystemExit(f"{name}: no seed satisfies the conditions")
        out.update({f"{name}_{k}": v for k, v in got.items()})
        print(f"{name}: seed {int(got['seed'])}, n = {got['pts2d'].shape[1]}, inliers per sample {got['mask'].sum(1).tolist()}")
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(HERE, "golden_pnp_robust.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
