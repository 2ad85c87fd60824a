"""Generate tests/golden/golden_pnp.npz: the reference's back-propagatable PnP (lib/utils/BPnP.py) on CPU.

Run by hand where the reference tree exists:  ``python tests/golden/gen_golden_pnp.py``

What is pinned, and by what:
  * the BACKWARD comes from the reference itself: ``BPnP_m3d.backward`` / ``BPnP.backward`` (BPnP.py:50-111, 154-236) through a
    hand-built ``ctx``, once in fp32 as it ships and once under ``torch.set_default_dtype(torch.float64)``.  The gap between the
    two runs is the noise floor, as for golden_full_eval_fp64.npz.
  * the FORWARD cannot run here: it calls cv2.solvePnP (EPnP, then iterative Levenberg-Marquardt), and cv2 is not installed.  The
    optimum ``P_6d`` is therefore the minimiser of the same objective - sum_i |x_i - pi(K, R(w) X_i + t)|^2, the objective of
    SOLVEPNP_ITERATIVE - found by ``scipy.optimize.least_squares(method="lm")`` in fp64 from the generating pose.  The forward is
    pinned by that objective and by exact recovery of the generating pose at sigma = 0.
  * ``R_ref`` is the reference's ``lib.utils.geometries.angle_axis_to_rotation_matrix`` of ``P_6d[:, :3]`` (4 x 4), and the
    ``small_*`` rows pin its first-order branch (theta^2 <= 1e-6), which no PnP case reaches.

Shims (the container has neither cv2 nor kornia): an empty ``cv2``; ``kornia.geometry.conversions`` whose
``axis_angle_to_rotation_matrix`` / ``angle_axis_to_rotation_matrix`` are the reference's own geometries.angle_axis_to_rotation_matrix
(the torchgeometry formula kornia ships: axis = w / (theta + 1e-6), first-order branch at theta^2 <= 1e-6); ``device="cuda"`` dropped
from torch.tensor / torch.zeros and torch.cuda.synchronize a no-op (BPnP.py:2, 212-214, 220).

Cases (3-D points: the reference's URDFRobot.get_keypoints_only_fk on seeded joint angles inside JOINT_BOUNDS; poses at
centroid depth 0.5-2.5 m, rotation angle 0.1-3.0 rad; DREAM-like intrinsics fx = fy ~ 615, principal point (320, 240)):
  panda_s0 / panda_s1 / panda_s3   panda, n = 7, B = 8, pixel noise sigma = 0 / 1 / 3 px    (BPnP_m3d)
  kuka_s1                          kuka, n = 8, B = 8, sigma = 1                              (BPnP_m3d)
  baxter_s1                        baxter, n = 17, B = 8, sigma = 1                           (BPnP_m3d)
  shared_s1                        panda, one joint configuration, pts3d [n, 3] shared by B = 8 views, sigma = 1   (BPnP)
Keys per case <c>: <c>_pts2d [B,n,2] f32, <c>_pts3d [B,n,3] or [n,3] f32, <c>_K [3,3] f32, <c>_P6d [B,6] f64 (optimum),
<c>_P6d_true [B,6] f64 (generating pose), <c>_R_ref [B,4,4] f64, <c>_grad_output [B,6] f32, <c>_gx32/_gz32/_gK32 (fp32 reference),
<c>_gx64/_gz64/_gK64 (fp64 reference), <c>_sigma, <c>_shared (0/1).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.setup()
import torch  # noqa: E402
from scipy.optimize import least_squares  # noqa: E402
from scipy.spatial.transform import Rotation  # noqa: E402

from lib.dataset.const import JOINT_BOUNDS  # noqa: E402
from lib.utils import geometries as ref_geo  # noqa: E402
from lib.utils.urdf_robot import URDFRobot  # noqa: E402


def _import_reference_bpnp():
    sys.modules["cv2"] = types.ModuleType("cv2")
    kn = types.ModuleType("kornia")
    kg = types.ModuleType("kornia.geometry")
    kc = types.ModuleType("kornia.geometry.conversions")
    kc.axis_angle_to_rotation_matrix = ref_geo.angle_axis_to_rotation_matrix
    kc.angle_axis_to_rotation_matrix = ref_geo.angle_axis_to_rotation_matrix
    kn.geometry, kg.conversions = kg, kc
    sys.modules.update({"kornia": kn, "kornia.geometry": kg, "kornia.geometry.conversions": kc})

    def strip_device(fn):
        def wrapped(*a, **k):
            if k.get("device") == "cuda":
                k.pop("device")
            return fn(*a, **k)
        return wrapped

    torch.tensor = strip_device(torch.tensor)
    torch.zeros = strip_device(torch.zeros)
    torch.cuda.synchronize = lambda *a, **k: None
    import importlib
    return importlib.import_module("lib.utils.BPnP")


BP = _import_reference_bpnp()


class _Ctx:
    def __init__(self, *saved):
        self.saved_tensors = saved


def ref_backward(fn, pts2d, pts3d, K, P6d, gout, dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        t = [torch.tensor(np.asarray(a), dtype=dtype) for a in (pts2d, P6d, pts3d, K, gout)]
        gx, gz, gK, _ = fn.backward(_Ctx(t[0], t[1], t[2], t[3]), t[4])
    finally:
        torch.set_default_dtype(old)
    return gx.double().numpy(), gz.double().numpy(), gK.double().numpy()


def project(P6d, X, K):
    R = Rotation.from_rotvec(P6d[:3]).as_matrix()
    c = X @ R.T + P6d[3:]
    p = c @ K.T
    return p[:, :2] / p[:, 2:3]


def solve_lm(x, X, K, init):
    r = least_squares(lambda p: (project(p, X, K) - x).ravel(), init, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                      max_nfev=20000)
    return r.x


def rand_pose(g, X, K):
    """rotation angle 0.1-3.0 rad about a random axis; the key-point centroid at depth 0.5-2.5 m near the optical axis;
    redrawn until every point lies >= 0.15 m in front of the camera and projects within 2000 px of the centre."""
    while True:
        ax = g.normal(size=3)
        ax /= np.linalg.norm(ax)
        w = ax * g.uniform(0.1, 3.0)
        R = Rotation.from_rotvec(w).as_matrix()
        d = g.uniform(0.5, 2.5)
        cen = np.array([g.uniform(-0.15, 0.15) * d, g.uniform(-0.1, 0.1) * d, d])
        t = cen - R @ X.mean(0)
        c = X @ R.T + t
        if c[:, 2].min() < 0.15:
            continue
        uv = project(np.concatenate([w, t]), X, K)
        if np.abs(uv - K[:2, 2]).max() > 2000:
            continue
        return np.concatenate([w, t])


def fk_points(robot_type, g, B):
    robot = URDFRobot(robot_type)
    b = np.array(JOINT_BOUNDS[robot_type], dtype=np.float64)
    q = (b[:, 0] + (b[:, 1] - b[:, 0]) * g.random((B, len(b)))).astype(np.float32)
    with torch.no_grad():
        X = robot.get_keypoints_only_fk(torch.tensor(q)).float().numpy()
    return X, q


def make_case(out, name, robot_type, sigma, seed, shared=False, B=8):
    g = np.random.Generator(np.random.PCG64(seed))
    X, q = fk_points(robot_type, g, 1 if shared else B)
    K = np.array([[g.uniform(605, 625), 0, 320], [0, 0, 240], [0, 0, 1]], np.float64)
    K[1, 1] = K[0, 0]
    K = K.astype(np.float32).astype(np.float64)
    n = X.shape[1]
    pts2d = np.zeros((B, n, 2), np.float32)
    P_true = np.zeros((B, 6))
    P_opt = np.zeros((B, 6))
    for i in range(B):
        Xi = X[0 if shared else i].astype(np.float64)
        P_true[i] = rand_pose(g, Xi, K)
        x = project(P_true[i], Xi, K) + g.normal(0, sigma, (n, 2)) if sigma > 0 else project(P_true[i], Xi, K)
        pts2d[i] = x.astype(np.float32)
        P_opt[i] = solve_lm(pts2d[i].astype(np.float64), Xi, K, P_true[i])
    pts3d = X[0] if shared else X
    gout = g.normal(size=(B, 6)).astype(np.float32)
    fn = BP.BPnP if shared else BP.BPnP_m3d
    K32 = K.astype(np.float32)
    gx32, gz32, gK32 = ref_backward(fn, pts2d, pts3d, K32, P_opt.astype(np.float32), gout, torch.float32)
    gx64, gz64, gK64 = ref_backward(fn, pts2d, pts3d, K32, P_opt, gout, torch.float64)
    with torch.no_grad():
        R_ref = ref_geo.angle_axis_to_rotation_matrix(torch.tensor(P_opt[:, :3])).numpy()
    c = name
    out.update({f"{c}_pts2d": pts2d, f"{c}_pts3d": pts3d.astype(np.float32), f"{c}_K": K32, f"{c}_P6d": P_opt,
                f"{c}_P6d_true": P_true, f"{c}_R_ref": R_ref, f"{c}_grad_output": gout, f"{c}_q": q,
                f"{c}_gx32": gx32, f"{c}_gz32": gz32, f"{c}_gK32": gK32, f"{c}_gx64": gx64, f"{c}_gz64": gz64, f"{c}_gK64": gK64,
                f"{c}_sigma": np.float64(sigma), f"{c}_shared": np.int32(shared)})
    fl = [np.abs(a - b).max() / np.abs(b).max() for a, b in ((gx32, gx64), (gz32, gz64), (gK32, gK64))]
    rec = np.abs(P_opt - P_true).max()
    print(f"{c}: n={n} B={B} sigma={sigma}  |P_opt - P_true|max {rec:.2e}  fp32-vs-fp64 rel gap x {fl[0]:.2e} z {fl[1]:.2e} K {fl[2]:.2e}")


def main():
    torch.set_num_threads(8)
    out = {}
    cases = [("panda_s0", "panda", 0.0, 11, False), ("panda_s1", "panda", 1.0, 12, False), ("panda_s3", "panda", 3.0, 13, False),
             ("kuka_s1", "kuka", 1.0, 14, False), ("baxter_s1", "baxter", 1.0, 15, False), ("shared_s1", "panda", 1.0, 16, True)]
    for name, rt, sig, seed, shared in cases:
        make_case(out, name, rt, sig, seed, shared)
    out["cases"] = np.array([c[0] for c in cases])
    # rotation-only rows of angle_axis_to_rotation_matrix: both sides of theta^2 = 1e-6, zero included
    g = np.random.Generator(np.random.PCG64(17))
    ax = g.normal(size=(8, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    th = np.array([0.0, 1e-5, 1e-4, 5e-4, 9.9e-4, 1.01e-3, 2e-3, 0.5])
    small = (ax * th[:, None]).astype(np.float32)
    with torch.no_grad():
        out["small_aa"] = small
        out["small_R_ref"] = ref_geo.angle_axis_to_rotation_matrix(torch.tensor(small)).numpy()
        out["small_R_ref64"] = ref_geo.angle_axis_to_rotation_matrix(torch.tensor(small, dtype=torch.float64)).numpy()
    path = os.path.join(HERE, "golden_pnp.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
