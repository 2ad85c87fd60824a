"""Kinematic refit: joint angles and, optionally, the camera pose from 2-D key-points (``hrp_kin_solve``, csrc/kin_core.h).

Nothing in the reference estimates the joint state from image evidence at inference (scripts/test.py only has the ``known_joint``
switch).  Two uses:

* a calibrated camera without encoders: ``KinematicRefit(robot, "fixed_camera", cTr=CalibrationResult.cTr)`` solves the joint
  angles of every frame with the pose fixed;
* the two heads of ``RootNetwithRegInt`` meeting at inference: ``KinematicRefit(robot, "holistic", prior_q=...)`` refits the
  regressor's ``(pose, rot, trans)`` to the integral head's key-points, so the reported pose reprojects onto them.

Which joints CAN be solved is a property of the robot and its key-points: a joint whose axis carries every key-point downstream of
it moves none of them (``observable_joints``), and a joint that moves all key-points as one rigid body is absorbed by the camera pose
when that is free too (an exact gauge).  ``kin_solve`` refuses both unless a prior (or fixing the joint) removes the freedom.  There
is no robust loss: on this problem an outlier on a distal key-point is simply fitted by the distal joints, and a Huber loss at 3 px
gave the L2 answer in 8 of 9 CPU experiments; the prior, the joint limits and per-point weights are what protects the estimate -
and, over a sequence, ``KinematicFilter`` below, whose gate knows where the arm was a frame ago.
With several fixed, calibrated cameras on one arm, ``kin_solve_views`` / ``MultiViewRefit`` (``hrp_kin_solve_views``,
csrc/kin_views_core.h) solve the joints once from all views: a second camera lowers the joint error about tenfold.
Over a recorded sequence, or with a lag of a few frames, ``KinematicFilter.smooth`` / ``kin_smooth`` (``hrp_kin_smooth``,
csrc/kin_smooth_core.h) run a Rauch-Tung-Striebel pass over the filter's posteriors: every frame then also knows its future.
There is no CPU path: CPU tensors raise HrpError.  No backward."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from hrpe_amd import _native as nv
from hrpe_amd.lib.dataset.const import JOINT_BOUNDS, JOINT_NAMES

KinResult = namedtuple("KinResult", "q rot trans kp3d kp2d rms status cov")

_PROBE_FRACTIONS = ((0.3, 0.55, 0.7), (0.65, 0.35, 0.5), (0.45, 0.7, 0.3))      # of [lo, hi], cycled over the joints
_PROBE_STEP = 1e-4
_MOVES = 1e-9            # metres per unit: a column below this is zero (the exact ones are ~1e-17, the smallest real one ~1e-2)


# ---- float64 FK on the host, from the chain tables --------------------------------------------------------------------------------------
def chain_tables(chain):
    """The ctypes hrp_fk_chain as numpy arrays (float64 copies of its fp32 tables)."""
    nj, nkp = int(chain.njoints), int(chain.nkp)
    a = lambda f, n, dt: np.array([f[i] for i in range(n)], dtype=dt)      # noqa: E731
    return dict(nj=nj, nkp=nkp, dof=int(chain.dof), parent=a(chain.parent, nj, np.int64), type=a(chain.type, nj, np.int64),
                cfg=a(chain.cfg, nj, np.int64), mul=a(chain.mimic_mul, nj, np.float64), off=a(chain.mimic_off, nj, np.float64),
                origin=np.array([[chain.origin[i][k] for k in range(12)] for i in range(nj)], dtype=np.float64).reshape(nj, 3, 4),
                axis=np.array([[chain.axis[i][k] for k in range(3)] for i in range(nj)], dtype=np.float64).reshape(nj, 3),
                kp_frame=a(chain.kp_frame, nkp, np.int64),
                kp_offset=np.array([[chain.kp_offset[k][r] for r in range(3)] for k in range(nkp)], dtype=np.float64).reshape(nkp, 3))


def _axis_rotation(a, q):
    s, c = np.sin(q), np.cos(q)
    sk = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return c * np.eye(3) + (1.0 - c) * np.outer(a, a) + s * sk


def fk_frames(tab, q):
    """Base-frame pose [nj, 4, 4] of every joint's child frame at q [dof], float64 (T = T_parent origin Rot(axis, q))."""
    T = np.zeros((tab["nj"], 4, 4))
    for j in range(tab["nj"]):
        O = np.eye(4)
        O[:3] = tab["origin"][j]
        M = np.eye(4)
        cfg = tab["cfg"][j]
        if tab["type"][j] != 0 and 0 <= cfg < tab["dof"]:
            qv = tab["mul"][j] * q[cfg] + tab["off"][j]
            if tab["type"][j] == 1:
                M[:3, :3] = _axis_rotation(tab["axis"][j], qv)
            else:
                M[:3, 3] = tab["axis"][j] * qv
        P = np.eye(4) if tab["parent"][j] < 0 else T[tab["parent"][j]]
        T[j] = P @ O @ M
    return T


def fk_points(tab, q):
    """Base-frame key-points [nkp, 3] at q [dof], float64."""
    T = fk_frames(tab, np.asarray(q, dtype=np.float64))
    out = np.zeros((tab["nkp"], 3))
    for k in range(tab["nkp"]):
        F = np.eye(4) if tab["kp_frame"][k] < 0 else T[tab["kp_frame"][k]]
        out[k] = F[:3, :3] @ tab["kp_offset"][k] + F[:3, 3]
    return out


def _bounds(robot):
    b = JOINT_BOUNDS.get(getattr(robot, "robot_type", None))
    dof = int(robot.chain.dof)
    if b is None or len(b) != dof:
        return np.full(dof, -1.0), np.full(dof, 1.0)
    b = np.asarray(b, dtype=np.float64)
    return b[:, 0], b[:, 1]


def _sensitivity(robot):
    """(observable [dof] bool, rigid [dof] bool), cached on the robot: central differences of the float64 host FK at three fixed
    configurations inside the joint bounds.  observable: the joint moves at least one key-point.  rigid: at every configuration the
    joint moves ALL key-points as one rigid body (dX_k = a x X_k + b for one (a, b)), which a free camera pose absorbs exactly."""
    cached = getattr(robot, "_kin_sensitivity", None)
    if cached is not None:
        return cached
    tab = chain_tables(robot.chain)
    dof, nkp = tab["dof"], tab["nkp"]
    lo, hi = _bounds(robot)
    obs, rigid = np.zeros(dof, bool), np.ones(dof, bool)
    for fr in _PROBE_FRACTIONS:
        q = np.array([lo[j] + fr[j % 3] * (hi[j] - lo[j]) for j in range(dof)])
        X = fk_points(tab, q)
        # dX = a x X + b, linear in (a, b): rows [-[X]x | I]
        A = np.zeros((3 * nkp, 6))
        for k in range(nkp):
            x = X[k]
            A[3 * k:3 * k + 3, :3] = -np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]])
            A[3 * k:3 * k + 3, 3:] = np.eye(3)
        for j in range(dof):
            d = np.zeros(dof)
            d[j] = _PROBE_STEP
            col = ((fk_points(tab, q + d) - fk_points(tab, q - d)) / (2.0 * _PROBE_STEP)).ravel()
            moves = np.abs(col).max() > _MOVES
            obs[j] |= moves
            res = col - A @ np.linalg.lstsq(A, col, rcond=None)[0]
            rigid[j] &= bool(moves and np.abs(res).max() < 1e-6 * max(1.0, np.abs(col).max()))
    robot._kin_sensitivity = (obs, rigid & obs)
    return robot._kin_sensitivity


def observable_joints(robot):
    """Host bool [dof]: True where the joint moves at least one key-point.  Panda: joint 7 and the finger do not (link7 and the hand
    origin lie on joint 7's axis); Kuka: joint 7; Baxter: head_pan and both w2."""
    return _sensitivity(robot)[0].copy()


def gauge_joints(robot):
    """Host bool [dof]: True where the joint moves all key-points as one rigid body, so that a free camera pose absorbs it (Panda and
    Kuka: joint 1, which turns about the base z axis through key-point 0)."""
    return _sensitivity(robot)[1].copy()


def _joint_name(robot, j):
    names = JOINT_NAMES.get(getattr(robot, "robot_type", None), [])
    return f"joint {j} ({names[j]})" if j < len(names) else f"joint {j}"


def _host_vector(v, dof, what):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise nv.HrpError(f"kin_solve: {what} is checked on the host before anything is launched: pass host values, not a GPU tensor")
        v = v.detach().numpy()
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(dof, float(a))
    if a.shape != (dof,):
        raise nv.HrpError(f"kin_solve: {what} {a.shape}, want a number or [{dof}]")
    return a


def _constant_on(robot, dev, values):
    """A host vector as a device tensor, uploaded once per (device, values) and kept on the robot like ``chain_on``'s chain."""
    cache = robot.__dict__.setdefault("_kin_consts", {})
    key = (str(dev), values.astype(np.float32).tobytes())
    if key not in cache:
        cache[key] = torch.from_numpy(values.astype(np.float32)).to(dev)
    return cache[key]


def resolve_free(robot, free_joints, free_pose, prior_q):
    """The host half of kin_solve: (free mask [dof] bool, prior [dof] float64 or None) or HrpError.  Runs before any GPU call."""
    dof = int(robot.chain.dof)
    obs, rigid = _sensitivity(robot)
    prior = _host_vector(prior_q, dof, "prior_q")
    if prior is not None and (not np.isfinite(prior).all() or (prior < 0).any()):
        raise nv.HrpError("kin_solve: prior_q must be finite and >= 0")
    has_prior = np.zeros(dof, bool) if prior is None else prior > 0
    if free_joints is None:
        free = obs & ~(rigid & ~has_prior) if free_pose else obs.copy()
    else:
        f = np.asarray(free_joints)
        if f.dtype == bool:
            if f.shape != (dof,):
                raise nv.HrpError(f"kin_solve: free_joints mask {f.shape}, want [{dof}]")
            free = f.copy()
        else:
            idx = f.astype(np.int64).ravel()
            if idx.size and (idx.min() < 0 or idx.max() >= dof):
                raise nv.HrpError(f"kin_solve: free_joints index outside [0, {dof})")
            free = np.zeros(dof, bool)
            free[idx] = True
        for j in np.flatnonzero(free & ~obs & ~has_prior):
            raise nv.HrpError(f"kin_solve: {_joint_name(robot, j)} moves no key-point (unobservable): give it a prior or do not free it")
        if free_pose:
            for j in np.flatnonzero(free & rigid & ~has_prior):
                raise nv.HrpError(f"kin_solve: {_joint_name(robot, j)} moves all key-points as one rigid body, an exact gauge with "
                                  "the free camera pose: give it a prior or do not free it")
    return free, prior


def _dev32(t, shapes, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise nv.HrpError(f"kin_solve: {what} must be a GPU tensor (there is no CPU path)")
    if tuple(t.shape) not in shapes:
        raise nv.HrpError(f"kin_solve: {what} {tuple(t.shape)}, want {' or '.join(str(s) for s in shapes)}")
    return t.detach().float().contiguous()


def kin_solve(robot, pts2d, K, q0, rot0, trans0, *, free_joints=None, free_pose=True, root=0, w2d=None, pts3d=None, w3d=None,
              prior_q=None, limits=True):
    """One launch: LM on the free joints (and the pose) of every sample from q0 / rot0 / trans0.

    pts2d [B, nkp, 2]; K [3, 3] or [B, 3, 3]; q0 [B, dof]; rot0 [B, 3 | 6] or [3 | 6] (one pose for all) with trans0 [B, 3] or [3];
    free_joints: bool mask [dof] or joint indices, None = ``observable_joints`` (without the gauge joints when the pose is free and
    they have no prior); w2d [B, nkp] >= 0; pts3d [B, nkp, 3] with w3d [B, nkp] (px^2 / m^2): optional camera-frame targets;
    prior_q: HOST number or [dof], px^2 per rad^2 (m^2 for a prismatic joint), pulls q to q0; limits: True = JOINT_BOUNDS, False, or
    a host (lo [dof], hi [dof]).  Returns KinResult(q, rot, trans, kp3d, kp2d, rms [B], status [B, 4] int32 = (flags
    _native.KIN_*, LM trials, rows, npar), cov [B, npar, npar]); see include/hrp.h for the exact semantics.  Asking for a free joint
    that is unobservable, or one that is a gauge of the free pose, without a prior raises HrpError naming the joint.  Does not
    synchronise, keeps no state between calls (constants are uploaded once and cached on the robot) and can be captured in a graph
    after one call outside it."""
    dof, nkp = int(robot.chain.dof), int(robot.chain.nkp)
    free, prior = resolve_free(robot, free_joints, free_pose, prior_q)
    if not 0 <= int(root) < nkp:
        raise nv.HrpError(f"kin_solve: root {root!r}, want 0 .. {nkp - 1}")
    lo = hi = None
    if limits is True:
        if getattr(robot, "robot_type", None) not in JOINT_BOUNDS:
            raise nv.HrpError("kin_solve: limits=True needs a robot with JOINT_BOUNDS; pass (lo, hi) or limits=False")
        lo, hi = _bounds(robot)
    elif limits not in (False, None):
        lo, hi = (_host_vector(v, dof, "limits") for v in limits)
    if (pts3d is None) != (w3d is None):
        raise nv.HrpError("kin_solve: pts3d and w3d go together")
    if not isinstance(pts2d, torch.Tensor) or pts2d.dim() != 3:
        raise nv.HrpError("kin_solve: pts2d must be a GPU tensor [B, nkp, 2] (there is no CPU path)")
    B = int(pts2d.shape[0])
    x = _dev32(pts2d, [(B, nkp, 2)], "pts2d")
    dev = x.device
    k = _dev32(K, [(3, 3), (B, 3, 3)], "K")
    q = _dev32(q0, [(B, dof)], "q0")
    r = _dev32(rot0, [(B, 3), (B, 6), (3,), (6,)], "rot0")
    t = _dev32(trans0, [(B, 3)] if r.dim() == 2 else [(3,)], "trans0")
    w2 = None if w2d is None else _dev32(w2d, [(B, nkp)], "w2d")
    x3 = None if pts3d is None else _dev32(pts3d, [(B, nkp, 3)], "pts3d")
    w3 = None if w3d is None else _dev32(w3d, [(B, nkp)], "w3d")
    rot_dim, shared = int(r.shape[-1]), r.dim() == 1
    npar = int(free.sum()) + (6 if free_pose else 0)
    consts = [None if v is None else _constant_on(robot, dev, v) for v in (lo, hi, prior)]
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)      # noqa: E731
    res = KinResult(q=new(B, dof), rot=new(B, rot_dim), trans=new(B, 3), kp3d=new(B, nkp, 3), kp2d=new(B, nkp, 2), rms=new(B),
                    status=new(B, 4, dt=torch.int32), cov=new(B, npar, npar))
    ptr = lambda v: None if v is None else v.data_ptr()      # noqa: E731
    d = nv.KinDesc()
    d.chain, d.pts2d, d.w2d, d.pts3d, d.w3d = robot.chain_on(dev).data_ptr(), x.data_ptr(), ptr(w2), ptr(x3), ptr(w3)
    d.K, d.K_stride, d.nkp, d.dof = k.data_ptr(), 0 if k.dim() == 2 else 9, nkp, dof
    d.q0, d.rot0, d.trans0, d.rot_dim, d.pose_stride = q.data_ptr(), r.data_ptr(), t.data_ptr(), rot_dim, 0 if shared else 1
    d.q_lo, d.q_hi, d.prior_q = (ptr(v) for v in consts)
    d.free_q, d.free_pose, d.root, d.B = int(sum(1 << int(j) for j in np.flatnonzero(free))), 1 if free_pose else 0, int(root), B
    d.q, d.rot, d.trans, d.xyz, d.uv = res.q.data_ptr(), res.rot.data_ptr(), res.trans.data_ptr(), res.kp3d.data_ptr(), res.kp2d.data_ptr()
    d.rms, d.status, d.cov = res.rms.data_ptr(), res.status.data_ptr(), res.cov.data_ptr()
    nv.call("hrp_kin_solve", C.byref(d), torch.cuda.current_stream(dev).cuda_stream)
    return res


class KinematicRefit:
    """The options of a refit, held for a stream of calls (``PoseTracker(..., refit=...)`` or ``solve`` directly).

    mode="holistic": the pose and the observable joints are free, every free joint has a prior, root = reference_keypoint_id: the
    network's ``(pose, rot, trans)`` is the start and the prior mean.  ``prior_q`` is REQUIRED: px^2 per rad^2 (per m^2 for a
    prismatic joint), a host number or [dof].  It weighs one radian of disagreement with the regressor against one pixel of
    reprojection error; no value has been tuned on a trained network (no checkpoint exists in this tree), so there is no default
    that would pretend to be measured.
    mode="fixed_camera": ``cTr`` [6] (angle-axis then translation, ``CalibrationResult.cTr``) is the one fixed pose of every sample
    (root = 0), and only the joints are solved; prior_q is optional."""

    def __init__(self, robot, mode, prior_q=None, cTr=None, free_joints=None, limits=True, reference_keypoint_id=3):
        if mode not in ("holistic", "fixed_camera"):
            raise nv.HrpError(f"KinematicRefit: mode {mode!r}, want 'holistic' or 'fixed_camera'")
        if mode == "holistic":
            if prior_q is None:
                raise nv.HrpError("KinematicRefit: mode 'holistic' needs prior_q (px^2 per rad^2); there is no tuned default")
            if cTr is not None:
                raise nv.HrpError("KinematicRefit: cTr belongs to mode 'fixed_camera'")
        elif cTr is None:
            raise nv.HrpError("KinematicRefit: mode 'fixed_camera' needs cTr [6] (CalibrationResult.cTr)")
        self.robot, self.mode, self.limits = robot, mode, limits
        self.free_pose = mode == "holistic"
        self.root = int(reference_keypoint_id) if self.free_pose else 0
        self.free, prior = resolve_free(robot, free_joints, self.free_pose, prior_q)
        if self.free_pose and (prior[self.free] <= 0).any():
            raise nv.HrpError("KinematicRefit: mode 'holistic' wants a prior > 0 on every free joint")
        self.prior_q = prior
        self.cTr = None
        if cTr is not None:
            c = cTr.detach().double().cpu().numpy() if isinstance(cTr, torch.Tensor) else np.asarray(cTr, dtype=np.float64)
            if c.shape != (6,) or not np.isfinite(c).all():
                raise nv.HrpError(f"KinematicRefit: cTr {c.shape}, want 6 finite numbers (angle-axis, translation)")
            self.cTr = c

    def solve(self, pts2d, K, pose, rot=None, trans=None, w2d=None, pts3d=None, w3d=None):
        """kin_solve with the held options from ``pose`` [B, dof] (and ``rot`` / ``trans`` in holistic mode)."""
        if self.free_pose:
            if rot is None or trans is None:
                raise nv.HrpError("KinematicRefit.solve: mode 'holistic' starts from the network's rot and trans")
            if not isinstance(rot, torch.Tensor) or rot.shape[-1] not in (3, 6):
                raise nv.HrpError("KinematicRefit.solve: the rotation must be angle-axis [B, 3] or two rows of R [B, 6]")
        else:
            if not isinstance(pose, torch.Tensor) or not pose.is_cuda:
                raise nv.HrpError("kin_solve: q0 must be a GPU tensor (there is no CPU path)")
            c = _constant_on(self.robot, pose.device, self.cTr)
            rot, trans = c[:3], c[3:]
        return kin_solve(self.robot, pts2d, K, pose, rot, trans, free_joints=self.free, free_pose=self.free_pose, root=self.root,
                         w2d=w2d, pts3d=pts3d, w3d=w3d, prior_q=self.prior_q, limits=self.limits)


# ---- several fixed cameras ------------------------------------------------------------------------------------------------------------------
KinViewsResult = namedtuple("KinViewsResult", "q rms rms_view used_view status cov kp3d kp2d")


def kin_solve_views(robot, pts2d, K, poses, q0, *, free_joints=None, w2d=None, prior_q=None, limits=True, want_cov=True):
    """One launch (``hrp_kin_solve_views``, csrc/kin_views_core.h): LM on the free joints of every sample over the key-points seen
    by V fixed, calibrated cameras at once, from q0.

    pts2d [B, V, nkp, 2]; K [V, 3, 3] (shared over the batch) or [B, V, 3, 3]; poses [V, 6] or [B, V, 6]: camera from base, angle-axis
    then translation, the ``cTr`` of ``CameraCalibrator.solve()``; q0 [B, dof]; free_joints: bool mask [dof] or joint indices, None =
    ``observable_joints``; w2d [B, V, nkp] >= 0; prior_q and limits as ``kin_solve``'s.  The camera poses are fixed, so no joint is
    a gauge here and none needs a prior for that; an unobservable free joint without a prior raises HrpError naming the joint.
    Returns KinViewsResult(q [B, dof], rms [B] over all used points, rms_view [B, V], used_view [B, V] int32, status [B, 4] int32 =
    (flags _native.KIN_*, LM trials, rows, npar), cov [B, npar, npar] (None with want_cov=False), kp3d [B, V, nkp, 3] camera-frame
    key-points of every view at q, kp2d [B, V, nkp, 2]); see include/hrp.h for the exact semantics.  Does not synchronise, keeps no state
    between calls (constants are uploaded once and cached on the robot) and can be captured in a graph after one call outside it."""
    dof, nkp = int(robot.chain.dof), int(robot.chain.nkp)
    free, prior = resolve_free(robot, free_joints, False, prior_q)
    lo = hi = None
    if limits is True:
        if getattr(robot, "robot_type", None) not in JOINT_BOUNDS:
            raise nv.HrpError("kin_solve_views: limits=True needs a robot with JOINT_BOUNDS; pass (lo, hi) or limits=False")
        lo, hi = _bounds(robot)
    elif limits not in (False, None):
        lo, hi = (_host_vector(v, dof, "limits") for v in limits)
    if not isinstance(pts2d, torch.Tensor) or pts2d.dim() != 4:
        raise nv.HrpError("kin_solve_views: pts2d must be a GPU tensor [B, V, nkp, 2] (there is no CPU path)")
    B, V = int(pts2d.shape[0]), int(pts2d.shape[1])
    if not 1 <= V <= nv.KIN_MAX_VIEWS:
        raise nv.HrpError(f"kin_solve_views: {V} views, want 1 .. {nv.KIN_MAX_VIEWS}")
    x = _dev32(pts2d, [(B, V, nkp, 2)], "pts2d")
    dev = x.device
    k = _dev32(K, [(V, 3, 3), (B, V, 3, 3)], "K")
    c = _dev32(poses, [(V, 6), (B, V, 6)], "poses")
    q = _dev32(q0, [(B, dof)], "q0")
    w2 = None if w2d is None else _dev32(w2d, [(B, V, nkp)], "w2d")
    npar = int(free.sum())
    consts = [None if v is None else _constant_on(robot, dev, v) for v in (lo, hi, prior)]
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)      # noqa: E731
    res = KinViewsResult(q=new(B, dof), rms=new(B), rms_view=new(B, V), used_view=new(B, V, dt=torch.int32), status=new(B, 4, dt=torch.int32),
                         cov=new(B, npar, npar) if want_cov else None, kp3d=new(B, V, nkp, 3), kp2d=new(B, V, nkp, 2))
    ptr = lambda v: None if v is None else v.data_ptr()      # noqa: E731
    d = nv.KinViewsDesc()
    d.chain, d.pts2d, d.w2d = robot.chain_on(dev).data_ptr(), x.data_ptr(), ptr(w2)
    d.K, d.K_stride, d.nkp, d.q0 = k.data_ptr(), 0 if k.dim() == 3 else 9, nkp, q.data_ptr()
    d.poses, d.pose_stride, d.V = c.data_ptr(), 0 if c.dim() == 2 else 1, V
    d.q_lo, d.q_hi, d.prior_q = (ptr(v) for v in consts)
    d.free_q, d.B, d.dof = int(sum(1 << int(j) for j in np.flatnonzero(free))), B, dof
    d.q, d.xyz, d.uv, d.rms, d.rms_view = res.q.data_ptr(), res.kp3d.data_ptr(), res.kp2d.data_ptr(), res.rms.data_ptr(), res.rms_view.data_ptr()
    d.status, d.used_view, d.cov = res.status.data_ptr(), res.used_view.data_ptr(), ptr(res.cov)
    nv.call("hrp_kin_solve_views", C.byref(d), torch.cuda.current_stream(dev).cuda_stream)
    return res


def _rotation_of(w):
    th = float(np.linalg.norm(w))
    return np.eye(3) if th < 1e-300 else _axis_rotation(w / th, th)


class MultiViewRefit:
    """The options of a multi-view refit, held for a stream of calls (``PoseTracker(..., streams=V, refit=...)`` or ``solve`` directly):
    V fixed, calibrated cameras on one arm, joints only (``mode`` = "multi_view").

    cTr: [V, 6] (angle-axis then translation per camera), or a list of V entries, each a ``CalibrationResult`` (its ``cTr``), a tensor
    or 6 numbers.  prior_q, free_joints and limits as ``kin_solve_views``'; prior_q is optional - no value has been tuned.  ``views``
    is V; ``rot3`` [V, 3], ``rot6`` [V, 6] (two rows of R) and ``trans`` [V, 3] are the cameras' poses in both of the model's rotation
    representations, computed on the host here."""
    mode = "multi_view"

    def __init__(self, robot, cTr, prior_q=None, free_joints=None, limits=True):
        rows = cTr if isinstance(cTr, (list, tuple)) else [cTr]
        rows = [getattr(r, "cTr", r) for r in rows]
        rows = [r.detach().double().cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r, dtype=np.float64) for r in rows]
        try:
            c = np.concatenate([r.reshape(-1, 6) for r in rows])
        except ValueError:
            raise nv.HrpError("MultiViewRefit: cTr must be [V, 6] or a list of V poses of 6 numbers (angle-axis, translation)") from None
        if not 1 <= len(c) <= nv.KIN_MAX_VIEWS:
            raise nv.HrpError(f"MultiViewRefit: {len(c)} views, want 1 .. {nv.KIN_MAX_VIEWS}")
        if not np.isfinite(c).all():
            raise nv.HrpError("MultiViewRefit: cTr must be finite")
        self.robot, self.limits, self.cTr, self.views = robot, limits, c, len(c)
        self.free, self.prior_q = resolve_free(robot, free_joints, False, prior_q)
        self.rot3, self.trans = c[:, :3].copy(), c[:, 3:].copy()
        self.rot6 = np.stack([_rotation_of(w)[:2].ravel() for w in self.rot3])

    def solve(self, kp2d, K, q_guess, w2d=None):
        """kin_solve_views with the held options: kp2d [B, V, nkp, 2], K [V, 3, 3] or [B, V, 3, 3], q_guess [B, dof]."""
        if not isinstance(q_guess, torch.Tensor) or not q_guess.is_cuda:
            raise nv.HrpError("kin_solve: q0 must be a GPU tensor (there is no CPU path)")
        poses = _constant_on(self.robot, q_guess.device, self.cTr.ravel()).view(self.views, 6)
        return kin_solve_views(self.robot, kp2d, K, poses, q_guess, free_joints=self.free, w2d=w2d, prior_q=self.prior_q, limits=self.limits)

    def pose_on(self, dev, rot_dim):
        """(rot [V, rot_dim], trans [V, 3]) on the device, uploaded once."""
        if rot_dim not in (3, 6):
            raise nv.HrpError(f"MultiViewRefit: rotation of {rot_dim} numbers, want 3 (angle-axis) or 6 (two rows of R)")
        rot = self.rot3 if rot_dim == 3 else self.rot6
        return _constant_on(self.robot, dev, rot.ravel()).view(self.views, rot_dim), _constant_on(self.robot, dev, self.trans.ravel()).view(self.views, 3)


# ---- the kinematic filter -------------------------------------------------------------------------------------------------------------------
KinFilterResult = namedtuple("KinFilterResult", "q rot trans kp3d kp2d vel cov kp3d_next status d2")
KinHistory = namedtuple("KinHistory", "mean cov valid flags dt q_in")
KinSmoothResult = namedtuple("KinSmoothResult", "q rot trans vel cov kp3d status mean cov_full", defaults=(None, None))


def _positive_vector(v, n, what, strict):
    if v is None:
        raise nv.HrpError(f"KinematicFilter: {what} is required (a host number or [{n}]); there is no tuned default")
    a = _host_vector(v, n, what)
    if not np.isfinite(a).all() or ((a <= 0).any() if strict else (a < 0).any()):
        raise nv.HrpError(f"KinematicFilter: {what} must be finite and {'> 0' if strict else '>= 0'}")
    return a


class KinematicFilter:
    """``kin_solve``'s parameters tracked over frames (``hrp_kin_filter_step``, csrc/kin_filter_core.h): a constant-velocity prior on
    (p, v), an innovation gate on the key-points and one launch per frame.  What a per-frame refit cannot do follows from the state:
    an outlier on a distal key-point is far from where the arm was a frame ago and is gated out; a frame without key-points is
    coasted; the covariance is written on a joint limit too.

    mode is one of ``KinematicRefit``'s: "holistic" (the pose and the observable joints are free, root = reference_keypoint_id, the
    network's ``(pose, rot, trans)`` is where a stream starts) or "fixed_camera" (``cTr`` [6] is the one fixed pose, root = 0).  A
    gauge joint needs no prior here: the state prior regularises it.  An unobservable free joint is refused by name unless w_q
    measures it.
    dt: seconds per frame.  q_acc: white-noise acceleration density per parameter, (rad or m)^2 s^-4, a host number or [n];
    p0_var: the variances a stream starts with, (p, v), a host number or [2n]; w_q: optional weight of the regressor's joints as a
    direct measurement, rad^-2 (m^-2), a host number or [dof]; gate_chi2: None = no gate; max_coast: frames without a usable point
    before a stream is lost.  n = free joints + 6 (holistic) <= _native.KIN_FILTER_MAX_N.  q_acc and p0_var are REQUIRED, and w_q
    and gate_chi2 are off unless given: nothing has been tuned on a trained network (no checkpoint exists in this tree), so there
    is no default that would pretend to be.
    The object owns the state (``mean`` [streams, 2n] and ``cov`` [streams, 2n, 2n] float64, ``valid`` and ``coast`` int32), created
    on the device of the first ``step``; ``reset`` clears ``valid``.  Nothing here synchronises; a step can be captured in a graph
    after one call outside it.  The additive pose model holds away from |w| = pi (include/hrp.h).
    ``history`` (an attribute, 0 by default: nothing is recorded and a step issues exactly one launch): with ``flt.history = T`` the
    filter owns a device ring of T slots (``KinHistory``: mean [T, streams, 2n] and cov [T, streams, 2n, 2n] float64, valid and flags
    [T, streams] int32, dt [T] float64, q_in [T, streams, dof] float32) and every step is followed by one more launch,
    ``hrp_kin_history_push``, that copies the posterior, the step's flags, its ``pose`` input and its dt into the next slot.  The slot
    cursor lives on the host; nothing synchronises.  ``smooth`` runs the RTS pass over what is recorded, ``clear_history`` empties the
    ring, ``reset`` starts the streams again (their next frame is INIT, which cuts the link).  A recording step and ``smooth`` raise
    HrpError while the current stream is capturing a graph: the slot and the length would be baked into it."""

    def __init__(self, robot, mode, dt, q_acc, p0_var, streams=1, cTr=None, free_joints=None, limits=True, gate_chi2=None, max_coast=5,
                 w_q=None, reference_keypoint_id=3):
        if mode not in ("holistic", "fixed_camera"):
            raise nv.HrpError(f"KinematicFilter: mode {mode!r}, want 'holistic' or 'fixed_camera'")
        if mode == "holistic" and cTr is not None:
            raise nv.HrpError("KinematicFilter: cTr belongs to mode 'fixed_camera'")
        if mode == "fixed_camera" and cTr is None:
            raise nv.HrpError("KinematicFilter: mode 'fixed_camera' needs cTr [6] (CalibrationResult.cTr)")
        self.robot, self.mode, self.free_pose = robot, mode, mode == "holistic"
        self.root = int(reference_keypoint_id) if self.free_pose else 0
        self.dof, self.nkp = int(robot.chain.dof), int(robot.chain.nkp)
        if not 0 <= self.root < self.nkp:
            raise nv.HrpError(f"KinematicFilter: reference_keypoint_id {reference_keypoint_id!r}, want 0 .. {self.nkp - 1}")
        # the gauge check does not apply (free_pose=False below): the state prior removes that freedom
        self.free, self.w_q = resolve_free(robot, free_joints, False, w_q)
        self.n = int(self.free.sum()) + (6 if self.free_pose else 0)
        if not 1 <= self.n <= nv.KIN_FILTER_MAX_N:
            raise nv.HrpError(f"KinematicFilter: {self.n} parameters, want 1 .. {nv.KIN_FILTER_MAX_N}")
        self.dt = self._dt(dt)
        self.q_acc = _positive_vector(q_acc, self.n, "q_acc", False)
        self.p0_var = _positive_vector(p0_var, 2 * self.n, "p0_var", True)
        self.gate_chi2 = 0.0 if gate_chi2 is None else float(gate_chi2)
        if gate_chi2 is not None and not (np.isfinite(self.gate_chi2) and self.gate_chi2 > 0):
            raise nv.HrpError(f"KinematicFilter: gate_chi2 {gate_chi2!r}, want a positive number or None (no gate)")
        if int(max_coast) != max_coast or int(max_coast) < 0:
            raise nv.HrpError(f"KinematicFilter: max_coast {max_coast!r}, want an integer >= 0")
        self.max_coast, self.B = int(max_coast), int(streams)
        if self.B < 1:
            raise nv.HrpError(f"KinematicFilter: {streams!r} streams")
        self.lo = self.hi = None
        if limits is True:
            if getattr(robot, "robot_type", None) not in JOINT_BOUNDS:
                raise nv.HrpError("KinematicFilter: limits=True needs a robot with JOINT_BOUNDS; pass (lo, hi) or limits=False")
            self.lo, self.hi = _bounds(robot)
        elif limits not in (False, None):
            self.lo, self.hi = (_host_vector(v, self.dof, "limits") for v in limits)
        self.cTr = None
        if cTr is not None:
            c = cTr.detach().double().cpu().numpy() if isinstance(cTr, torch.Tensor) else np.asarray(cTr, dtype=np.float64)
            if c.shape != (6,) or not np.isfinite(c).all():
                raise nv.HrpError(f"KinematicFilter: cTr {c.shape}, want 6 finite numbers (angle-axis, translation)")
            self.cTr = c
        self.mean = self.cov = self.valid = self.coast = None
        self._acc = self._var = None
        self._hist_cap = self._hist_len = self._hist_next = 0
        self._hist = self._hist_rot_dim = None

    @property
    def history(self):
        """Slots of the recorded history (0: nothing is recorded).  Setting another size empties the ring."""
        return self._hist_cap

    @history.setter
    def history(self, slots):
        if isinstance(slots, bool) or int(slots) != slots or int(slots) < 0:
            raise nv.HrpError(f"KinematicFilter: history {slots!r}, want an integer >= 0")
        if int(slots) != self._hist_cap:
            self._hist_cap, self._hist = int(slots), None
            self.clear_history()

    def clear_history(self):
        """Forget what was recorded (the ring's memory is kept)."""
        self._hist_len = self._hist_next = 0

    def recorded(self):
        """(KinHistory, first, length): the ring's tensors as they lie (not copies), the slot of the oldest recorded frame and the
        number of frames recorded: what ``kin_smooth`` takes.  (None, 0, 0) before the first recording step."""
        if self._hist is None:
            return None, 0, 0
        return self._hist, (self._hist_next - self._hist_len) % self._hist_cap, self._hist_len

    def _history_on(self, dev, rot_dim):
        if self._hist is None:
            T, B, N = self._hist_cap, self.B, 2 * self.n
            z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
            self._hist = KinHistory(mean=z(T, B, N, dt=torch.float64), cov=z(T, B, N, N, dt=torch.float64), valid=z(T, B, dt=torch.int32),
                                    flags=z(T, B, dt=torch.int32), dt=z(T, dt=torch.float64), q_in=z(T, B, self.dof, dt=torch.float32))
            self._hist_rot_dim = rot_dim
        elif self._hist_rot_dim != rot_dim:
            raise nv.HrpError(f"KinematicFilter: the history was recorded with rot_dim {self._hist_rot_dim}, this step has {rot_dim}")

    def _push(self, q, status, step_dt, dev):
        h = self._hist
        d = nv.KinHistoryDesc()
        d.mean, d.cov, d.valid, d.status, d.q_in = self.mean.data_ptr(), self.cov.data_ptr(), self.valid.data_ptr(), status.data_ptr(), q.data_ptr()
        d.h_mean, d.h_cov, d.h_valid, d.h_flags, d.h_dt, d.h_q_in = (v.data_ptr() for v in (h.mean, h.cov, h.valid, h.flags, h.dt, h.q_in))
        d.B, d.n, d.dof, d.cap, d.slot, d.dt = self.B, self.n, self.dof, self._hist_cap, self._hist_next, step_dt
        nv.call("hrp_kin_history_push", C.byref(d), torch.cuda.current_stream(dev).cuda_stream)
        self._hist_next = (self._hist_next + 1) % self._hist_cap
        self._hist_len = min(self._hist_len + 1, self._hist_cap)

    def smooth(self, lag=None, cov=True, full=False):
        """The RTS pass over the newest ``lag`` recorded frames (None: all of them), two launches.  Returns KinSmoothResult(q [L, B, dof],
        rot, trans, vel [L, B, n], cov [L, B, n, n] (None with cov=False), kp3d [L, B, nkp, 3], status [L, B, 2] int32 = (flags
        _native.KS_*, later frames that reached this one), and with full=True mean [L, B, 2n] and cov_full [L, B, 2n, 2n] float64), oldest
        frame first.  ``smooth(lag=k)`` is the last k rows of ``smooth()``, byte for byte; cov=False skips the covariance recursion
        and leaves the other outputs' bytes as they are.  See include/hrp.h for the exact semantics."""
        if self._hist_cap < 1:
            raise nv.HrpError("KinematicFilter.smooth: nothing is recorded (set history = T before the steps)")
        if self._hist_len < 1 or self._hist is None:
            raise nv.HrpError("KinematicFilter.smooth: the history is empty")
        L = self._hist_len if lag is None else lag
        if isinstance(L, bool) or int(L) != L or not 1 <= int(L) <= self._hist_len:
            raise nv.HrpError(f"KinematicFilter.smooth: lag {lag!r}, want 1 .. {self._hist_len} (the frames recorded)")
        dev = self._hist.mean.device
        pose = None
        if not self.free_pose:
            c = _constant_on(self.robot, dev, self.cTr)
            pose = (c[:3], c[3:])
        limits = False if self.lo is None else (self.lo, self.hi)
        return kin_smooth(self.robot, self._hist, self.q_acc, self.free, free_pose=self.free_pose, root=self.root, pose=pose,
                          rot_dim=self._hist_rot_dim, limits=limits, first=(self._hist_next - int(L)) % self._hist_cap, length=int(L),
                          cov=cov, full=full)

    @staticmethod
    def _dt(dt):
        if isinstance(dt, torch.Tensor) or not np.isfinite(float(dt)) or not float(dt) > 0:
            raise nv.HrpError(f"KinematicFilter: dt {dt!r}, want a positive, finite host number (seconds)")
        return float(dt)

    def _state_on(self, dev):
        if self.mean is None:
            z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
            self.mean, self.cov = z(self.B, 2 * self.n, dt=torch.float64), z(self.B, 2 * self.n, 2 * self.n, dt=torch.float64)
            self.valid, self.coast = z(self.B, dt=torch.int32), z(self.B, dt=torch.int32)
            self._acc, self._var = torch.from_numpy(self.q_acc).to(dev), torch.from_numpy(self.p0_var).to(dev)
        elif self.mean.device != dev:
            raise nv.HrpError(f"KinematicFilter: the state lives on {self.mean.device}, the inputs on {dev}")

    def reset(self, streams=None):
        """Clear ``valid``: the streams (all, or the given indices) start again at their next step."""
        if self.valid is None:
            return
        if streams is None:
            self.valid.zero_()
        else:
            self.valid.index_fill_(0, torch.as_tensor(list(streams), dtype=torch.int64).to(self.valid.device), 0)

    def step(self, pts2d, K, pose, rot=None, trans=None, w2d=None, q_meas=None, keep=None, dt=None):
        """One frame, one launch.  pts2d [B, nkp, 2]; K [3, 3] or [B, 3, 3]; pose [B, dof]: where a stream starts and the fixed joints
        of every frame; rot [B, 3 | 6] and trans [B, 3] in holistic mode; w2d [B, nkp]: inverse variances in px^-2 (None = 1); q_meas
        [B, dof]: the joints' measurement, read when w_q is set (None = pose); keep [B] int32: 0 starts the stream again; dt: this
        frame's step when it differs from the constructor's.  Returns KinFilterResult(q, rot, trans, kp3d, kp2d, vel [B, n], cov
        [B, n, n], kp3d_next (FK at p + dt v), status [B, 4] int32 = (flags _native.KF_*, LM trials, points used, points gated),
        d2 [B, nkp]); see include/hrp.h for the exact semantics."""
        B, dof, nkp, n = self.B, self.dof, self.nkp, self.n
        step_dt = self.dt if dt is None else self._dt(dt)
        if self.free_pose:
            if rot is None or trans is None:
                raise nv.HrpError("KinematicFilter.step: mode 'holistic' starts from the network's rot and trans")
            if not isinstance(rot, torch.Tensor) or rot.shape[-1] not in (3, 6):
                raise nv.HrpError("KinematicFilter.step: the rotation must be angle-axis [B, 3] or two rows of R [B, 6]")
        elif rot is not None or trans is not None:
            raise nv.HrpError("KinematicFilter.step: mode 'fixed_camera' takes its pose from cTr")
        x = _dev32(pts2d, [(B, nkp, 2)], "pts2d")
        dev = x.device
        if self._hist_cap and torch.cuda.is_current_stream_capturing():
            raise nv.HrpError("KinematicFilter.step: a step that records its history cannot be captured in a graph (the ring's slot "
                              "would be baked into it); set history = 0 for the captured filter")
        k = _dev32(K, [(3, 3), (B, 3, 3)], "K")
        q = _dev32(pose, [(B, dof)], "pose")
        if self.free_pose:
            r = _dev32(rot, [(B, 3), (B, 6)], "rot")
            t = _dev32(trans, [(B, 3)], "trans")
        else:
            c = _constant_on(self.robot, dev, self.cTr)
            r, t = c[:3], c[3:]
        w2 = None if w2d is None else _dev32(w2d, [(B, nkp)], "w2d")
        qm = None
        if self.w_q is not None:
            qm = q if q_meas is None else _dev32(q_meas, [(B, dof)], "q_meas")
        if keep is not None:
            if not isinstance(keep, torch.Tensor) or not keep.is_cuda or keep.dtype != torch.int32 or tuple(keep.shape) != (B,):
                raise nv.HrpError(f"KinematicFilter.step: keep must be an int32 GPU tensor [{B}]")
            keep = keep.contiguous()
        self._state_on(dev)
        rot_dim = int(r.shape[-1])
        if self._hist_cap:
            self._history_on(dev, rot_dim)
        consts = [None if v is None else _constant_on(self.robot, dev, v) for v in (self.lo, self.hi, self.w_q)]
        new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)      # noqa: E731
        res = KinFilterResult(q=new(B, dof), rot=new(B, rot_dim), trans=new(B, 3), kp3d=new(B, nkp, 3), kp2d=new(B, nkp, 2), vel=new(B, n),
                              cov=new(B, n, n), kp3d_next=new(B, nkp, 3), status=new(B, 4, dt=torch.int32), d2=new(B, nkp))
        ptr = lambda v: None if v is None else v.data_ptr()      # noqa: E731
        d = nv.KinFilterDesc()
        d.chain, d.pts2d, d.w2d = self.robot.chain_on(dev).data_ptr(), x.data_ptr(), ptr(w2)
        d.K, d.K_stride, d.nkp, d.dof = k.data_ptr(), 0 if k.dim() == 2 else 9, nkp, dof
        d.q_in, d.rot_in, d.trans_in, d.rot_dim, d.pose_stride = q.data_ptr(), r.data_ptr(), t.data_ptr(), rot_dim, 1 if self.free_pose else 0
        d.q_lo, d.q_hi, d.w_q = (ptr(v) for v in consts)
        d.q_meas, d.keep, d.q_acc, d.p0_var = ptr(qm), ptr(keep), self._acc.data_ptr(), self._var.data_ptr()
        d.free_q, d.free_pose, d.root, d.B = int(sum(1 << int(j) for j in np.flatnonzero(self.free))), 1 if self.free_pose else 0, self.root, B
        d.max_coast, d.dt, d.gate_chi2 = self.max_coast, step_dt, self.gate_chi2
        d.mean, d.cov, d.valid, d.coast = self.mean.data_ptr(), self.cov.data_ptr(), self.valid.data_ptr(), self.coast.data_ptr()
        d.q, d.rot, d.trans, d.xyz, d.uv = res.q.data_ptr(), res.rot.data_ptr(), res.trans.data_ptr(), res.kp3d.data_ptr(), res.kp2d.data_ptr()
        d.vel, d.cov_p, d.xyz_next, d.d2, d.status = (res.vel.data_ptr(), res.cov.data_ptr(), res.kp3d_next.data_ptr(), res.d2.data_ptr(),
                                                      res.status.data_ptr())
        nv.call("hrp_kin_filter_step", C.byref(d), torch.cuda.current_stream(dev).cuda_stream)
        if self._hist_cap:
            self._push(q, res.status, step_dt, dev)
        return res


# ---- the kinematic smoother -----------------------------------------------------------------------------------------------------------------
def _scratch_on(robot, dev, gain, link):
    """The links' scratch (gain fp64, link int32), kept on the robot per device and grown when a call needs more.  Calls that overlap
    on two streams of one device would share it: smooth on one stream at a time."""
    cache = robot.__dict__.setdefault("_kin_smooth_scratch", {})
    g, l = cache.get(str(dev), (None, None))
    if g is None or g.numel() < gain or l.numel() < link:
        g = torch.empty(max(gain, 0 if g is None else g.numel()), dtype=torch.float64, device=dev)
        l = torch.empty(max(link, 0 if l is None else l.numel()), dtype=torch.int32, device=dev)
        cache[str(dev)] = (g, l)
    return g, l


def kin_smooth(robot, history, q_acc, free, *, free_pose, root=0, pose=None, rot_dim=3, limits=True, first=0, length=None, cov=True,
               full=False):
    """``hrp_kin_smooth`` on explicit history tensors: the Rauch-Tung-Striebel pass of ``KinematicFilter.smooth``.

    history: KinHistory(mean [cap, B, 2n] and cov [cap, B, 2n, 2n] float64, valid and flags [cap, B] int32 (flags: the filter step's
    _native.KF_*), dt [cap] float64, q_in [cap, B, dof] float32), GPU tensors, the ring as it lies: frame t = 0 .. length-1 (oldest
    first) is slot (first + t) % cap; length None = cap.  q_acc: HOST [n], the filter's; free: HOST bool mask [dof] of the joints in
    the state (no observability check: nothing is measured here); free_pose: the state ends with (w, t); pose: (rot [rot_dim], trans [3])
    GPU tensors, the fixed pose when free_pose is False; rot_dim: of the rot output; limits as ``kin_solve``'s.  Returns
    KinSmoothResult; see ``KinematicFilter.smooth`` and include/hrp.h.  Two launches, no synchronisation; raises HrpError while the
    current stream is capturing a graph."""
    dof, nkp = int(robot.chain.dof), int(robot.chain.nkp)
    free = np.asarray(free)
    if free.dtype != bool or free.shape != (dof,):
        raise nv.HrpError(f"kin_smooth: free must be a bool mask [{dof}]")
    n = int(free.sum()) + (6 if free_pose else 0)
    if not 1 <= n <= nv.KIN_FILTER_MAX_N:
        raise nv.HrpError(f"kin_smooth: {n} parameters, want 1 .. {nv.KIN_FILTER_MAX_N}")
    acc = _host_vector(q_acc, n, "q_acc")
    if acc is None or not np.isfinite(acc).all() or (acc < 0).any():
        raise nv.HrpError("kin_smooth: q_acc must be finite and >= 0")
    if not 0 <= int(root) < nkp:
        raise nv.HrpError(f"kin_smooth: root {root!r}, want 0 .. {nkp - 1}")
    if rot_dim not in (3, 6):
        raise nv.HrpError(f"kin_smooth: rot_dim {rot_dim!r}, want 3 or 6")
    lo = hi = None
    if limits is True:
        if getattr(robot, "robot_type", None) not in JOINT_BOUNDS:
            raise nv.HrpError("kin_smooth: limits=True needs a robot with JOINT_BOUNDS; pass (lo, hi) or limits=False")
        lo, hi = _bounds(robot)
    elif limits not in (False, None):
        lo, hi = (_host_vector(v, dof, "limits") for v in limits)
    h = KinHistory(*history)
    if not isinstance(h.mean, torch.Tensor) or not h.mean.is_cuda or h.mean.dim() != 3:
        raise nv.HrpError("kin_smooth: history.mean must be a GPU tensor [cap, B, 2n] (there is no CPU path)")
    cap, B, N = int(h.mean.shape[0]), int(h.mean.shape[1]), 2 * n
    dev = h.mean.device
    for name, want, dt in (("mean", (cap, B, N), torch.float64), ("cov", (cap, B, N, N), torch.float64), ("valid", (cap, B), torch.int32),
                           ("flags", (cap, B), torch.int32), ("dt", (cap,), torch.float64), ("q_in", (cap, B, dof), torch.float32)):
        v = getattr(h, name)
        if not isinstance(v, torch.Tensor) or v.device != dev or v.dtype != dt or tuple(v.shape) != want or not v.is_contiguous():
            raise nv.HrpError(f"kin_smooth: history.{name} must be a contiguous {dt} tensor {want} on {dev}")
    L = cap if length is None else int(length)
    if not 1 <= L <= cap or not 0 <= int(first) < cap or B < 1:
        raise nv.HrpError(f"kin_smooth: length {length!r} / first {first!r}, want 1 <= length <= cap = {cap} and 0 <= first < cap")
    if free_pose:
        if pose is not None:
            raise nv.HrpError("kin_smooth: pose is the fixed pose of free_pose=False")
        rf = tf = None
    else:
        if pose is None:
            raise nv.HrpError("kin_smooth: free_pose=False needs pose = (rot, trans)")
        rf, tf = _dev32(pose[0], [(rot_dim,)], "pose[0]"), _dev32(pose[1], [(3,)], "pose[1]")
    if torch.cuda.is_current_stream_capturing():
        raise nv.HrpError("kin_smooth: cannot be captured in a graph (the ring's start and length would be baked into it)")
    consts = [None if v is None else _constant_on(robot, dev, v) for v in (lo, hi)]
    cache = robot.__dict__.setdefault("_kin_consts64", {})
    key = (str(dev), acc.tobytes())
    if key not in cache:
        cache[key] = torch.from_numpy(acc.copy()).to(dev)
    gain, link = _scratch_on(robot, dev, L * B * N * N, L * B)
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)      # noqa: E731
    res = KinSmoothResult(q=new(L, B, dof), rot=new(L, B, rot_dim), trans=new(L, B, 3), vel=new(L, B, n), cov=new(L, B, n, n) if cov else None,
                          kp3d=new(L, B, nkp, 3), status=new(L, B, 2, dt=torch.int32), mean=new(L, B, N, dt=torch.float64) if full else None,
                          cov_full=new(L, B, N, N, dt=torch.float64) if full and cov else None)
    ptr = lambda v: None if v is None else v.data_ptr()      # noqa: E731
    d = nv.KinSmoothDesc()
    d.chain, d.mean, d.cov, d.valid, d.flags, d.dt, d.q_in = (robot.chain_on(dev).data_ptr(), h.mean.data_ptr(), h.cov.data_ptr(),
                                                               h.valid.data_ptr(), h.flags.data_ptr(), h.dt.data_ptr(), h.q_in.data_ptr())
    d.rot_fixed, d.trans_fixed, d.q_lo, d.q_hi, d.q_acc = ptr(rf), ptr(tf), ptr(consts[0]), ptr(consts[1]), cache[key].data_ptr()
    d.gain, d.link = gain.data_ptr(), link.data_ptr()
    d.free_q, d.free_pose, d.root, d.B = int(sum(1 << int(j) for j in np.flatnonzero(free))), 1 if free_pose else 0, int(root), B
    d.dof, d.nkp, d.rot_dim, d.cap, d.first, d.L, d.want_cov = dof, nkp, rot_dim, cap, int(first), L, 1 if cov else 0
    d.q, d.rot, d.trans, d.vel, d.cov_p, d.xyz = (res.q.data_ptr(), res.rot.data_ptr(), res.trans.data_ptr(), res.vel.data_ptr(), ptr(res.cov),
                                                  res.kp3d.data_ptr())
    d.status, d.mean_s, d.cov_s = res.status.data_ptr(), ptr(res.mean), ptr(res.cov_full)
    nv.call("hrp_kin_smooth", C.byref(d), torch.cuda.current_stream(dev).cuda_stream)
    return res
