"""``CtRNet`` (reference lib/models/ctrnet/CtRNet.py:10-129): the key-point / segmentation predictor behind a DataParallel-shaped
wrapper (the reference's checkpoints carry the ``module.`` prefix), the detection entry points and the pose from them:

* ``inference_batch_images_onlyseg`` (102-111), the mask network's call, unchanged;
* ``inference_batch_images_seg_kp`` (91-100): key-points and foreground probability from one plan;
* ``inference_batch_images`` / ``inference_single_image`` (49-89): the same, plus ``cTr`` from the GPU PnP solver (``BPnP_m3d`` /
  ``BPnP``, lib/utils/BPnP.py, csrc/pnp.hip - the reference calls OpenCV on the host), or, with ``reproj_error`` given, from the
  robust solver (``BPnP_robust``: consensus over P3P hypotheses, LM on the inliers), the inlier mask kept as ``last_inliers``;
* ``inference_sequence``: ONE pose for a whole batch of frames of a fixed camera (``pnp_solve_pooled``, csrc/pnp_pooled.hip), where the
  reference has only the per-frame calls above;
* ``cTr_to_pose_matrix`` (114-124), ``to_valid_R_batch`` (126-129).

Not built: ``render_single_robot_mask`` and ``train_on_batch`` (131-194; training the key-point network is out of scope)."""
import os
import sys

import numpy as np
import torch

from hrpe_amd import _native as nv
from hrpe_amd.lib.utils.BPnP import BPnP, BPnP_m3d, BPnP_robust, pnp_solve_pooled
from hrpe_amd.lib.utils.geometries import angle_axis_to_rotation_matrix
from .keypoint_seg_resnet import KeyPointSegNet


class _DataParallelShape(torch.nn.Module):
    """``torch.nn.DataParallel(model, device_ids=[0])`` as a name: one process per GPU here, nothing to scatter."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *a, **k):
        return self.module(*a, **k)


class CtRNet(torch.nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.device = "cuda" if args.use_gpu else "cpu"
        self.keypoint_seg_predictor = _DataParallelShape(KeyPointSegNet(args, use_gpu=args.use_gpu))
        path = args.keypoint_seg_model_path
        if path is not None and os.path.exists(path):
            print("Loading keypoint segmentation model from {}".format(path))
            self.keypoint_seg_predictor.load_state_dict(torch.load(path, map_location="cpu"))
        elif path is not None and not getattr(args, "allow_random_seg_init", False):
            # the reference fails in torch.load (CtRNet.py:35): a relative default path (models/panda_segmentation/*.pth) resolved from
            # the wrong working directory must not leave train_sim2real self-training against random masks.  Tests and benchmarks on
            # synthetic weights opt in with args.allow_random_seg_init = True.
            raise FileNotFoundError(f"CtRNet: keypoint_seg_model_path {path!r} does not exist (set args.allow_random_seg_init = True to "
                                    "keep the random initialisation on purpose)")
        if args.use_gpu and torch.cuda.is_available():       # (the reference moves unconditionally; a build container has no GPU)
            self.keypoint_seg_predictor = self.keypoint_seg_predictor.cuda()
        self.keypoint_seg_predictor.eval()
        self.intrinsics = np.array([[args.fx, 0., args.px], [0., args.fy, args.py], [0., 0., 1.]])
        self.K = torch.tensor(self.intrinsics, device=self.device if torch.cuda.is_available() else "cpu", dtype=torch.float)

    def inference_batch_images_onlyseg(self, img):
        """img [B, 3, H, W] (normalised) -> foreground probability [B, 1, H, W] (CtRNet.py:102-111)"""
        _, segmentation = self.keypoint_seg_predictor(img)
        return torch.sigmoid(segmentation)

    def _seg_kp(self, img):
        return self.keypoint_seg_predictor(img, keypoints=True)

    def _points_3d(self, joint_angles, points_3d, batch):
        """The 3-D key-points the 2-D detections are paired with.  Default: ``self.robot.get_keypoints_only_fk(joint_angles)`` of a
        ``URDFRobot`` the CALLER assigns to ``self.robot`` (the reference never assigns ``self.robot`` either, and its
        ``get_joint_RT`` comes from roboticstoolbox, which is not in the reference tree); scripts/test.py:121-122 pairs the same FK
        key-points with ``BPnP_m3d``.  UNPINNED: whether the link origins CtRNet's checkpoints were trained on coincide with the
        DREAM key-point offsets of ``URDFRobot`` is not verified by anything in either tree; pass ``points_3d`` to choose."""
        if points_3d is not None:
            return points_3d
        robot = getattr(self, "robot", None)
        if robot is None:
            raise nv.HrpError("CtRNet: the pose needs 3-D key-points: assign a URDFRobot to `robot` (its get_keypoints_only_fk(joint_angles) "
                              "is used) or pass `points_3d`")
        q = torch.as_tensor(joint_angles, dtype=torch.float32, device=self.K.device)
        pts = robot.get_keypoints_only_fk(q if batch else q[None])
        return pts if batch else pts[0]

    def inference_batch_images_seg_kp(self, img):
        """img [B, 3, H, W] (normalised) -> (points_2d [B, k, 2] in pixels, foreground probability [B, 1, H, W]) (CtRNet.py:91-100)"""
        points_2d, segmentation = self._seg_kp(img)
        return points_2d, torch.sigmoid(segmentation)

    def _robust_pose(self, points_2d, pts, reproj_error):
        cTr, self.last_inliers = BPnP_robust.apply(points_2d, pts.to(points_2d.device), self.K, float(reproj_error))
        return cTr

    def inference_batch_images(self, img, joint_angles, points_3d=None, reproj_error=None):
        """img [B, 3, H, W], joint_angles [B, dof] -> (cTr [B, 6] angle-axis + translation from BPnP_m3d, points_2d [B, k, 2],
        foreground probability) (CtRNet.py:68-89).  points_3d [B, k, 3]: see ``_points_3d``.  reproj_error (px): cTr from
        ``BPnP_robust`` instead, a key-point farther than that from the consensus pose has no say; ``self.last_inliers`` [B, k] bool."""
        points_2d, segmentation = self._seg_kp(img)
        pts = self._points_3d(joint_angles, points_3d, True)
        if reproj_error is not None:
            cTr = self._robust_pose(points_2d, pts, reproj_error)
        else:
            cTr = BPnP_m3d.apply(points_2d, pts.to(points_2d.device), self.K)
        return cTr, points_2d, torch.sigmoid(segmentation)

    def inference_single_image(self, img, joint_angles, points_3d=None, reproj_error=None):
        """img [3, H, W], joint_angles [dof] -> (cTr [1, 6] from BPnP, points_2d [1, k, 2], foreground probability [1, 1, H, W])
        (CtRNet.py:49-66).  points_3d [k, 3]: see ``_points_3d``.  reproj_error: as ``inference_batch_images``."""
        points_2d, segmentation = self._seg_kp(img[None])
        pts = self._points_3d(joint_angles, points_3d, False)
        if reproj_error is not None:
            cTr = self._robust_pose(points_2d, pts, reproj_error)
        else:
            cTr = BPnP.apply(points_2d, pts.to(points_2d.device), self.K)
        return cTr, points_2d, torch.sigmoid(segmentation)

    def inference_sequence(self, img, joint_angles, points_3d=None, reproj_error=3.0):
        """img [F, 3, H, W] of a camera that does not move, joint_angles [F, dof] -> (cTr [1, 6]: one pose from all F x k key-points
        through the pooled robust solver, points_2d [F, k, 2], foreground probability).  points_3d [F, k, 3]: see ``_points_3d``.
        ``self.last_inliers`` [F, k] bool: the key-points within ``reproj_error`` px of cTr.  No gradient."""
        points_2d, segmentation = self._seg_kp(img)
        pts = self._points_3d(joint_angles, points_3d, True).to(points_2d.device)
        F, k = points_2d.shape[0], points_2d.shape[1]
        cTr, inliers, _, _, _ = pnp_solve_pooled(points_2d.reshape(1, F * k, 2), pts.reshape(1, F * k, 3), self.K,
                                                 reproj_error=float(reproj_error), want_cov=False)
        self.last_inliers = inliers.reshape(F, k)
        return cTr, points_2d, torch.sigmoid(segmentation)

    def cTr_to_pose_matrix(self, cTr):
        """cTr [B, 6] -> pose matrix [B, 4, 4] (CtRNet.py:114-124) with BPnP.py's own axis-angle conversion
        (lib/utils/geometries.angle_axis_to_rotation_matrix, the one tests/golden/golden_pnp.npz pins)."""
        bs = cTr.shape[0]
        pose = torch.zeros((bs, 4, 4), device=cTr.device, dtype=cTr.dtype)
        pose[:, :3, :3] = angle_axis_to_rotation_matrix(cTr[:, :3].reshape(bs, 3))[:, :3, :3]
        pose[:, :3, 3] = cTr[:, 3:]
        pose[:, 3, 3] = 1
        return pose

    def to_valid_R_batch(self, R):
        """The nearest orthogonal matrices of a batch of 3 x 3 matrices (CtRNet.py:126-129): U V^T of the SVD."""
        U, _, Vh = torch.linalg.svd(R)
        return torch.bmm(U, Vh)
