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


# ---- the kinematic filter -------------------------------------------------------------------------------------------------------------------
KinFilterResult = namedtuple("KinFilterResult", "q rot trans kp3d kp2d vel cov kp3d_next status d2")


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
    after one call outside it.  The additive pose model holds away from |w| = pi (include/hrp.h)."""

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
        return res
