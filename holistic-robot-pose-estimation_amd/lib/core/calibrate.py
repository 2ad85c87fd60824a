"""Fixed-camera (eye-to-hand) calibration: ONE camera-to-base transform from a whole sequence, the multi-frame PnP of DREAM.

The arm moves through F configurations under a camera bolted to the cell; every frame gives k detected key-points and, through the
encoders and forward kinematics, their k base-frame positions.  ``CameraCalibrator`` collects the frames in device buffers and
``solve()`` hands all F x k correspondences to the pooled robust solver (``pnp_solve_pooled``, csrc/pnp_pooled.hip) as one problem:
a frame whose detector sat on a distractor, or a single stray key-point, has no say in the pose, and the returned covariance tells
whether the sequence so far pins it.  Nothing here synchronises: ``add`` and ``solve`` only enqueue work, ``len()`` is a host integer,
and the caller reads ``status`` when they want to know.

    cal = CameraCalibrator(robot, K)
    for img, q in camera_loop():                       # q [1, dof] from the encoders
        kp, prob, ms = detector.detect(img)
        cal.add_detection(kp, ms, q, scale=detector.args.scale, min_peak=0.2)
    res = cal.solve()                                  # res.cTr [6], res.cov [6, 6], res.frame_inliers [F]
"""
from collections import namedtuple

import torch

from hrpe_amd import _native as nv
from hrpe_amd.lib.utils.BPnP import pnp_solve_pooled
from hrpe_amd.lib.utils.geometries import angle_axis_to_rotation_matrix

CalibrationResult = namedtuple("CalibrationResult", "cTr R t inliers frame_inliers rms cov status")


class CameraCalibrator:
    """Ring of ``capacity_frames`` frames of a robot with k key-points: points_2d [capacity, k, 2], points_3d [capacity, k, 3] and
    valid [capacity, k] on the device, written at a host-side cursor; once full, the oldest frames are overwritten.
    ``min_inliers`` None: a quarter of the points held at ``solve()``, at least 4."""

    def __init__(self, robot, K, capacity_frames=1024, reproj_error=3.0, min_inliers=None, max_hypotheses=1024, seed=0, device="cuda"):
        self.robot = robot
        self.device = torch.device(device)
        self.K = torch.as_tensor(K, dtype=torch.float32).to(self.device).reshape(3, 3).contiguous()
        self.k = int(robot.nkp)
        self.capacity = int(capacity_frames)
        if self.capacity < 1 or self.capacity * self.k > nv.PNP_POOLED_MAX_N:
            raise ValueError(f"CameraCalibrator: {self.capacity} frames of {self.k} key-points; the pooled solver takes "
                             f"1 <= frames * key-points <= {nv.PNP_POOLED_MAX_N}")
        self.reproj_error, self.min_inliers, self.max_hypotheses, self.seed = float(reproj_error), min_inliers, int(max_hypotheses), int(seed)
        self.points_2d = torch.zeros(self.capacity, self.k, 2, device=self.device)
        self.points_3d = torch.zeros(self.capacity, self.k, 3, device=self.device)
        self.valid = torch.zeros(self.capacity, self.k, dtype=torch.bool, device=self.device)
        self.reset()

    def reset(self):
        self._cursor, self._count = 0, 0

    def __len__(self):
        return self._count

    def add(self, points_2d, joint_angles, valid=None, points_3d=None):
        """points_2d [F, k, 2] in pixels of the image K belongs to, joint_angles [F, dof]; the base-frame key-points are
        ``robot.get_keypoints_only_fk(joint_angles)`` unless points_3d [F, k, 3] is given.  valid [F, k]: the usable key-points."""
        x = torch.as_tensor(points_2d, dtype=torch.float32, device=self.device)
        F = x.shape[0]
        if tuple(x.shape) != (F, self.k, 2):
            raise ValueError(f"CameraCalibrator.add: points_2d must be [F, {self.k}, 2], got {list(x.shape)}")
        if points_3d is None:
            q = torch.as_tensor(joint_angles, dtype=torch.float32, device=self.device)
            points_3d = self.robot.get_keypoints_only_fk(q)
        X = torch.as_tensor(points_3d, dtype=torch.float32, device=self.device).detach()
        if tuple(X.shape) != (F, self.k, 3):
            raise ValueError(f"CameraCalibrator.add: points_3d must be [{F}, {self.k}, 3], got {list(X.shape)}")
        if valid is None:
            v = torch.ones(F, self.k, dtype=torch.bool, device=self.device)
        else:
            v = torch.as_tensor(valid, device=self.device) != 0
            if tuple(v.shape) != (F, self.k):
                raise ValueError(f"CameraCalibrator.add: valid must be [{F}, {self.k}], got {list(v.shape)}")
        src = max(0, F - self.capacity)                     # more frames than the ring holds: the last `capacity` of them
        while src < F:
            run = min(F - src, self.capacity - self._cursor)
            dst = slice(self._cursor, self._cursor + run)
            self.points_2d[dst].copy_(x[src:src + run].detach())
            self.points_3d[dst].copy_(X[src:src + run])
            self.valid[dst].copy_(v[src:src + run])
            self._cursor = (self._cursor + run) % self.capacity
            self._count = min(self._count + run, self.capacity)
            src += run

    def add_detection(self, kp, ms, joint_angles, scale, min_peak=0.0):
        """``seg_mask_inference.detect``'s key-points kp [F, k, 2] (pixels of the resized image, so divided by ``scale``) and ms
        [F, k, 2]: a key-point is usable where its peak probability 1 / ms[..., 1] is at least ``min_peak``."""
        self.add(kp / scale, joint_angles, valid=(1.0 / ms[..., 1]) >= min_peak)

    def frames(self):
        """(points_2d [F, k, 2], points_3d [F, k, 3], valid [F, k]) of the frames held, oldest first."""
        bufs = (self.points_2d, self.points_3d, self.valid)
        if self._count < self.capacity:
            return tuple(b[:self._count] for b in bufs)
        if self._cursor == 0:
            return bufs
        return tuple(torch.cat((b[self._cursor:], b[:self._cursor])) for b in bufs)

    def solve(self, refine_all=False):
        """One pose from every key-point of the frames held (oldest first): CalibrationResult(cTr [6] angle-axis then translation,
        R [3, 3], t [3], inliers [F, k] bool, frame_inliers [F], rms, cov [6, 6], status [4]), all on the device."""
        F, k = self._count, self.k
        if F * k < 4:
            raise ValueError(f"CameraCalibrator.solve: {F} frames of {k} key-points held; the solver needs four points")
        x, X, v = self.frames()
        min_inliers = max(4, F * k // 4) if self.min_inliers is None else int(self.min_inliers)
        P, inl, status, rms, cov = pnp_solve_pooled(x.reshape(1, F * k, 2), X.reshape(1, F * k, 3), self.K, reproj_error=self.reproj_error,
                                                    valid=v.reshape(1, F * k), min_inliers=min_inliers,
                                                    max_hypotheses=self.max_hypotheses, seed=self.seed, refine_all=refine_all)
        inl = inl.reshape(F, k)
        R = angle_axis_to_rotation_matrix(P[:, :3])[0, :3, :3]
        return CalibrationResult(P[0], R, P[0, 3:], inl, inl.sum(1), rms[0], cov[0], status[0])
