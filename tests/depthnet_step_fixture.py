"""Shared by test_depthnet_step_host.py and test_gpu_depthnet_step.py: the fixture of the reference's DepthNet trainer
(tests/golden/golden_depthnet_step.npz, written by gen_golden_depthnet_step.py) as batches, ground truth and options."""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN

# the generator's RUNS: what depthnet_loss / farward_loss are called with
RUNS = {
    "l1": dict(depth_loss_func="l1", xy_loss_func=None, kps_need_depth=None),
    "mse": dict(depth_loss_func="mse", xy_loss_func=None, kps_need_depth=None),
    "xy_l1": dict(depth_loss_func="l1", xy_loss_func="l1", kps_need_depth=None),
    "xy_mse": dict(depth_loss_func="l1", xy_loss_func="mse", kps_need_depth=None),
    "mkp_l1": dict(depth_loss_func="l1", xy_loss_func=None, kps_need_depth=[1, 3, 5]),
    "mkp_mse": dict(depth_loss_func="mse", xy_loss_func=None, kps_need_depth=[1, 3, 5]),
}
LOSS_RTOL = 2e-5        # the project's tolerance for fixture loss terms (header of test_gpu_eval.py)
ERROR_ATOL = 2.4e-7     # 2 ulp of fp32 in [1, 2), the fixture's depth range
VAL_TAGS = ("rootz_loss", "mean_depth_error", "mean_x_error", "mean_y_error")


class Args(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_depthnet_step.npz")))


def sizes():
    return [int(b) for b in golden()["sizes"]]


def run_options(run):
    G = golden()
    o = dict(RUNS[run], reference_keypoint_id=int(G[f"{run}:opt:reference_keypoint_id"]))
    return o


def run_args(run):
    """The trainer's options of a run, as farward_loss / validate read them."""
    G, o = golden(), RUNS[run]
    return Args(urdf_robot_name="kuka", reference_keypoint_id=int(G[f"{run}:opt:reference_keypoint_id"]),
                use_extended_bbox=bool(G[f"{run}:opt:use_extended_bbox"]), use_origin_bbox=bool(G[f"{run}:opt:use_origin_bbox"]),
                depth_loss_func=o["depth_loss_func"], use_rootnet_xy_branch=o["xy_loss_func"] is not None,
                xy_loss_func=o["xy_loss_func"] or "mse", multi_kp=o["kps_need_depth"] is not None, kps_need_depth=o["kps_need_depth"])


def gt_of(run, part, i, device="cpu"):
    """dict(root_trans, kp3d, mask) of a batch as the reference's step forms it (train_depthnet.py:172-194, 247)."""
    G, ref = golden(), int(golden()[f"{run}:opt:reference_keypoint_id"])
    kp3d = torch.tensor(G[f"{part}{i}:kp3d"])
    root_trans = torch.tensor(G[f"{part}{i}:TCO"][:, :3, 3]) if ref == 0 else kp3d[:, ref]
    mask = torch.tensor(G[f"{part}{i}:mask"][:, ref])
    return {k: v.contiguous().to(device) for k, v in dict(root_trans=root_trans, kp3d=kp3d, mask=mask).items()}


def pred_of(run, part, i, device="cpu"):
    return torch.tensor(golden()[f"{run}:{part}{i}:pred"]).to(device)


def batch_of(part, i, seed=0):
    """A batch in the DreamDataset schema.  Its ``other`` view is poisoned: the DepthNet step reads the root view only."""
    G = golden()
    f = lambda k: torch.tensor(G[f"{part}{i}:{k}"])   # noqa: E731
    B = f("K").shape[0]
    g = torch.Generator().manual_seed(seed + i)
    images = torch.randint(0, 256, (B, 3, 8, 8), generator=g, dtype=torch.uint8)
    bad = lambda t: torch.full_like(t, float("nan"))   # noqa: E731
    return {
        "root": {"images": images, "K": f("K"), "bbox_strict_bounded": f("bbox_strict"), "bbox_gt2d_extended": f("bbox_extended"),
                 "keypoints_3d": f("kp3d"), "valid_mask_crop": f("mask")},
        "other": {"images": images.flip(0), "K": bad(f("K")), "bbox_strict_bounded": bad(f("bbox_strict")),
                  "bbox_gt2d_extended": bad(f("bbox_extended")), "keypoints_3d": bad(f("kp3d")), "valid_mask_crop": 1 - f("mask")},
        "TCO": f("TCO"), "K_original": f("K_original"), "bbox_strict_bounded_original": f("bbox_original"), "valid_mask": f("mask"),
    }


class StubModel(torch.nn.Module):
    """forward returns the recorded prediction of the batch it is called for (in loader order) and keeps the k_values it got."""

    def __init__(self, preds):
        super().__init__()
        self.preds, self.calls, self.k_values, self.inputs = preds, 0, [], []
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, images, k_values):
        out = self.preds[self.calls % len(self.preds)]
        self.calls += 1
        self.k_values.append(k_values)
        self.inputs.append(images)
        return out.clone()


class Recorder:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, epoch):
        assert tag not in self.scalars, tag
        self.scalars[tag] = (float(value), epoch)
