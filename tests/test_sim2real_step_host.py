"""CPU-only checks of the self-supervised trainer's step (lib/core/sim2real.py, csrc/sim2real_step.hip): the host-tensor path of
``sim2real_monitor`` against a float64 restatement of reference scripts/train_sim2real.py:313-400, ``worst_cases`` against the
reference's ``sorted()`` formula (:582-588), the descriptor's layout, export and argument checks, and the options the step refuses.

No fixture can come from the reference here (its step is a closure inside the script and needs pytorch3d, cv2 and CUDA): the float64
restatement below, ``reference_row``, is what the new terms are pinned against, in this file and in tests/test_gpu_sim2real_step.py.

Bound.  rtol 2e-5 on every term - the project's tolerance for hrp_pose_loss terms (golden_pose_loss.npz test).  The cases are built
so that this is a statement about the arithmetic and not about cancellation: 3-D errors of centimetres on metres, 2-D errors of
tens of pixels on coordinates of hundreds (an fp32 projection carries about 1e-4 px), and a mean translation error that lies far
from the 0.5 switch on either side."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv

ROW = ("loss", "loss_joint", "loss_rot", "loss_trans", "loss_uv", "loss_depth", "loss_error2d", "loss_error3d", "loss_mask",
       "loss_scale", "loss_iou", "loss_error3d_align")
COMPUTED = ("loss_joint", "loss_rot", "loss_trans", "loss_uv", "loss_depth", "loss_error2d", "loss_error3d")
RTOL = 2e-5


def reference_row(pred, gt, K, image_size, mask_terms=None):
    """train_sim2real.py:313-400 line by line in float64 (the shipped loss functions' branches), on the fp32 inputs widened.
    -> dict of the twelve values as Python floats."""
    f = lambda t: t.detach().cpu().double()   # noqa: E731
    pred_pose, pred_rot, pred_trans, pred_root_uv, pred_root_depth, pred_keypoints3d = [f(pred[i]) for i in (0, 1, 2, 3, 4, 7)]
    gt_pose, gt_root_rot, gt_root_trans, gt_root_uv = f(gt["pose"]), f(gt["root_rot"]), f(gt["root_trans"]), f(gt["root_uv"])
    gt_keypoints3d, gt_keypoints2d, valid_mask_crop = f(gt["kp3d"]), f(gt["kp2d"]), f(gt["mask"])
    other_K = f(K).reshape(-1, 3, 3)
    gt_root_depth = gt_root_trans[:, 2].unsqueeze(-1)                                                    # :208
    # :243 point_projection_from_3d_tensor (transforms.py:7-21): hnormalized(K @ loc.T).T per sample
    pred_keypoints2d_reproj = torch.stack([((Kb @ loc.T) / (Kb @ loc.T)[-1])[:-1].T for Kb, loc in zip(other_K, pred_keypoints3d)])
    MSELoss, L1Loss = torch.nn.MSELoss(), torch.nn.L1Loss()                                             # :313-315
    loss_pose = MSELoss(pred_pose, gt_pose)                                                              # :321-322
    loss_rot = MSELoss(pred_rot, gt_root_rot)                                                            # :330-331
    loss_depth = L1Loss(pred_root_depth, gt_root_depth)                                                  # :337-338
    error_root_uv = torch.norm((pred_root_uv - gt_root_uv) / image_size, dim=1)                          # :350-353
    loss_uv = torch.mean(error_root_uv)
    error_root_trans = torch.norm(pred_trans - gt_root_trans, dim=1)                                     # :363-370
    loss_trans = torch.mean(error_root_trans)
    if loss_trans > 5e-1:
        coeff = torch.exp(- 20.0 * error_root_trans).detach()
        error_root_trans = error_root_trans * coeff
        loss_trans = torch.mean(error_root_trans)
    error3d = torch.norm(pred_keypoints3d - gt_keypoints3d, dim=2)                                       # :374-377
    loss_error3d = torch.mean(error3d)
    size = torch.tensor([image_size, image_size], dtype=torch.float64).reshape(1, 1, 2)                  # :381-386
    pred_keypoints2d_reproj = pred_keypoints2d_reproj / size
    gt_keypoints2d = gt_keypoints2d / size
    error2d_reproj = torch.norm(pred_keypoints2d_reproj - gt_keypoints2d, dim=2)
    error2d_reproj = error2d_reproj * valid_mask_crop
    loss_error2d = torch.sum(error2d_reproj) / torch.sum(valid_mask_crop != 0)
    out = {"loss_joint": loss_pose, "loss_rot": loss_rot, "loss_uv": loss_uv, "loss_depth": loss_depth, "loss_trans": loss_trans,
           "loss_error2d": loss_error2d, "loss_error3d": loss_error3d}                                    # :395-400
    mt = [0.0] * 5 if mask_terms is None else [float(v) for v in mask_terms.detach().cpu()]
    out.update(loss=mt[0], loss_mask=mt[1], loss_iou=mt[2], loss_scale=mt[3], loss_error3d_align=mt[4])   # :399-402, 463-468
    return {k: float(v) for k, v in out.items()}


def make_case(B, P, J, seed, far=False, mask="zeros"):
    """Seeded predictions and ground truth of one step (host fp32): (pred 8-tuple, gt, K [B,3,3], image_size).
    far: translation errors of 0.6 - 1.4 m (batch mean > 0.5, the damped branch of :367), else centimetres.
    mask: 'ones' | 'zeros' (random zeros, image 0 masked out entirely when B > 1, the key-point of index 0 of the last image too) |
    'none' (all zero)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *sh: lo + (hi - lo) * torch.rand(*sh, generator=g)        # noqa: E731
    n = lambda *sh: torch.randn(*sh, generator=g)                                # noqa: E731
    S = 256.0
    K = torch.tensor([[400.0, 0, 128], [0, 400.0, 128], [0, 0, 1]]).repeat(B, 1, 1)
    K[:, 0, 0] *= u(0.8, 1.2, B)
    K[:, 1, 1] *= u(0.8, 1.2, B)
    K[:, 0, 2] += u(-20, 20, B)
    kp3d = torch.cat([u(-.3, .3, B, J, 1), u(-.3, .3, B, J, 1), u(1.0, 2.0, B, J, 1)], 2)
    h = torch.einsum("bij,bkj->bki", K, kp3d)
    kp2d = h[..., :2] / h[..., 2:3] + 2.0 * n(B, J, 2)
    root_trans = kp3d[:, min(3, J - 1)].clone()
    gt = dict(pose=u(-2.5, 2.5, B, P), root_rot=n(B, 6), root_trans=root_trans, root_uv=kp2d[:, min(3, J - 1)].clone(), kp3d=kp3d, kp2d=kp2d)
    if mask == "ones":
        m = torch.ones(B, J)
    elif mask == "none":
        m = torch.zeros(B, J)
    else:
        m = (torch.rand(B, J, generator=g) > 0.3).float()
        m[-1, 0], m[-1, J - 1] = 0.0, 1.0
        if B > 1:
            m[0] = 0.0
    gt["mask"] = m
    d = n(B, 3)
    d = d / d.norm(dim=1, keepdim=True) * (u(0.6, 1.4, B, 1) if far else u(0.01, 0.05, B, 1))
    xyz_fk = kp3d + 0.05 * n(B, J, 3)
    pred = (gt["pose"] + 0.2 * n(B, P), gt["root_rot"] + 0.1 * n(B, 6), root_trans + d, gt["root_uv"] + 15.0 * n(B, 2),
            root_trans[:, 2:3] + 0.05 * n(B, 1), torch.zeros(B, J, 3), kp3d + 0.05 * n(B, J, 3), xyz_fk)
    return pred, gt, K, S


def check_row(got, ref, what=""):
    """Every entry of a row (dict of tensors / floats, or a [12] tensor) within RTOL of the float64 reference; NaN where it has NaN."""
    if isinstance(got, torch.Tensor):
        got = {k: got[i] for i, k in enumerate(ROW)}
    for k in ROW:
        a, b = float(got[k]), ref[k]
        print(f"{what}{k}: {a!r} vs {b!r} (rel {abs(a - b) / abs(b) if b else abs(a - b):.2e})")
        assert np.isnan(a) == np.isnan(b), (what, k, a, b)
        if not np.isnan(b):
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=0.0, err_msg=what + k)


def host_projection(camera_K, points):
    h = torch.einsum("bij,bkj->bki", camera_K.to(points.dtype), points)
    return h[..., :2] / h[..., 2:3]


# ---- 1. the host-tensor path against float64 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,P,J,far,mask", [(1, 8, 7, False, "ones"), (3, 8, 7, False, "zeros"), (3, 8, 7, True, "zeros"),
                                            (5, 15, 17, True, "ones"), (4, 7, 8, False, "none")])
def test_host_path_matches_float64_restatement(B, P, J, far, mask):
    from hrpe_amd.lib.core import sim2real as S
    assert S.ROW == ROW and set(S.LOSS_KEYS) == set(ROW[1:]) and len(S.LOSS_KEYS) == 11
    pred, gt, K, size = make_case(B, P, J, seed=100 + B + J, far=far, mask=mask)
    mt = torch.tensor([0.75, 0.125, 0.5, 2.5, 0.0625])
    ref = reference_row(pred, gt, K, size, mt)
    e = torch.norm(pred[2] - gt["root_trans"], dim=1).mean()
    assert (float(e) > 0.55) == far and (far or float(e) < 0.1)                  # the side of the :367 switch the case is meant for
    row, terms = S.sim2real_monitor(pred, gt, K, size, mask_terms=mt)
    assert row.shape == (12,) and row.dtype == torch.float32 and tuple(terms) == ROW and not row.requires_grad
    check_row(row, ref)
    assert np.isnan(ref["loss_error2d"]) == (mask == "none") and all(np.isfinite(ref[k]) for k in ROW if k != "loss_error2d")
    # the five copied entries are the mask terms bit for bit; zero without them
    assert [float(row[i]) for i in (0, 8, 9, 10, 11)] == [0.75, 0.125, 2.5, 0.5, 0.0625]
    row0, _ = S.sim2real_monitor(pred, gt, K, size)
    assert [float(row0[i]) for i in (0, 8, 9, 10, 11)] == [0.0] * 5
    assert torch.equal(row0[1:8].nan_to_num(-7.0), row[1:8].nan_to_num(-7.0))


def test_loss_uv_is_the_unmasked_mean_not_function_py_s_masked_quotient(monkeypatch):
    """The root key-point of one image is masked out: the script's loss_uv (:350-353) still counts that image, function.py's
    (:231-235, ``full_loss_expr``) does not - on the same inputs the two differ, and the monitor gives the script's."""
    from hrpe_amd.lib.core import function as F
    from hrpe_amd.lib.core import sim2real as S
    monkeypatch.setattr(F, "point_projection_from_3d_tensor", host_projection)   # (the library's projection is a device kernel)
    pred, gt, K, size = make_case(4, 8, 7, seed=9, mask="ones")
    gt["mask"][2, 3] = 0.0
    _, masked = F.full_loss_expr(pred, gt, K, root=3, image_size=size)
    row, terms = S.sim2real_monitor(pred, gt, K, size)
    ref = reference_row(pred, gt, K, size)
    np.testing.assert_allclose(float(terms["loss_uv"]), ref["loss_uv"], rtol=RTOL)
    e = torch.norm((pred[3] - gt["root_uv"]).double() / size, dim=1)
    np.testing.assert_allclose(float(masked["loss_uv"]), float((e.sum() - e[2]) / 3), rtol=RTOL)
    assert abs(float(masked["loss_uv"]) - float(terms["loss_uv"])) > 1e-3 * ref["loss_uv"]
    # with the root key-point visible everywhere the two forms agree
    gt["mask"][2, 3] = 1.0
    _, unmasked = F.full_loss_expr(pred, gt, K, root=3, image_size=size)
    np.testing.assert_allclose(float(unmasked["loss_uv"]), ref["loss_uv"], rtol=RTOL)


def test_host_meters_and_rows():
    from hrpe_amd.lib.core import sim2real as S
    m = S.TrainMeters("cpu")
    rows = torch.full((3, 12), -1.0)
    acc, got = np.zeros(12), []
    for i in range(3):
        pred, gt, K, size = make_case(2, 8, 7, seed=40 + i, mask="ones")
        row, _ = S.sim2real_monitor(pred, gt, K, size, mask_terms=torch.full((5,), float(i)), meters=m, rows=rows, row_index=2 - i)
        acc = acc + row.double().numpy()
        got.append(row)
    assert np.array_equal(m.sum.numpy(), acc) and int(m.count) == 3
    assert all(torch.equal(rows[2 - i], got[i]) for i in range(3))
    means = m.read_and_reset()
    assert tuple(means) == ROW and [means[k] for k in ROW] == list(acc / 3)
    assert float(m.sum.abs().max()) == 0.0 and int(m.count) == 0
    with pytest.raises(nv.HrpError, match="capacity"):
        S.sim2real_monitor(pred, gt, K, size, rows=rows, row_index=3)


# ---- 2. worst_cases -------------------------------------------------------------------------------------------------------------

def reference_worst_cases(dis3d, idx):
    """train_sim2real.py:582-588 as it stands (IndexError below 96 images)."""
    alldis = {"dis3d": list(dis3d), "idx": list(idx)}
    assert len(alldis["idx"]) == len(alldis["dis3d"]), (len(alldis["idx"]), len(alldis["dis3d"]))
    result = [(alldis["dis3d"][i], alldis["idx"][i]) for i in range(len(alldis["idx"]))]
    result_ordered = sorted(result)
    errors_down = [item[0] for item in result_ordered][::-1]
    view_ids_down = [item[1] for item in result_ordered][::-1]
    errors_list = [errors_down[i] for i in np.arange(0, 100, 5)]
    view_ids_list = [view_ids_down[i] for i in np.arange(0, 100, 5)]
    return view_ids_list, errors_list


@pytest.mark.parametrize("n", [100, 137])
def test_worst_cases_match_the_reference_formula(n):
    from hrpe_amd.lib.core.sim2real import worst_cases
    g = np.random.Generator(np.random.PCG64(n))
    dis = np.round(g.uniform(0.0, 0.2, n), 2).astype(np.float32)          # two decimals: many ties, broken by the image id
    assert len(np.unique(dis)) < n // 2
    idx = g.permutation(n).astype(np.int64)
    ids, errs = worst_cases(dis, idx)
    rids, rerrs = reference_worst_cases(dis, idx)
    assert len(ids) == 20 and ids == [int(v) for v in rids] and errs == [float(v) for v in rerrs]
    assert errs == sorted(errs, reverse=True) and errs[0] == float(dis.max())


def test_worst_cases_are_cut_below_96_images():
    from hrpe_amd.lib.core.sim2real import worst_cases
    dis = np.array([0.3, 0.1, 0.2, 0.2, 0.5, 0.0, 0.4], np.float32)
    idx = np.array([10, 11, 12, 13, 14, 15, 16])
    with pytest.raises(IndexError):
        reference_worst_cases(dis, idx)
    ids, errs = worst_cases(dis, idx)
    assert ids == [14, 11] and errs == [float(np.float32(0.5)), float(np.float32(0.1))]      # positions 0 and 5 of the descending order
    assert worst_cases(dis[:5], idx[:5]) == ([14], [0.5])


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------

def test_monitor_struct_size_matches_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "hrp.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(hrp_sim2real_monitor_desc), offsetof(hrp_sim2real_monitor_desc, mask_terms),
         offsetof(hrp_sim2real_monitor_desc, B), offsetof(hrp_sim2real_monitor_desc, capacity));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    D = nv.Sim2RealMonitorDesc
    assert out == [C.sizeof(D), D.mask_terms.offset, D.B.offset, D.capacity.offset]


def test_monitor_symbol_is_exported_and_bound():
    assert hasattr(nv.lib(), "hrp_sim2real_monitor") and "hrp_sim2real_monitor" in nv.PROTOTYPES
    src = open(os.path.join(ROOT, "include", "hrp.h")).read()
    assert "int hrp_sim2real_monitor(const hrp_sim2real_monitor_desc* d, void* stream);" in src
    assert nv.SIM2REAL_ROW == ROW


def test_monitor_rejects_bad_descriptors_without_a_gpu():
    """hrp_sim2real_monitor validates on the host before it launches: every call here returns HRP_ERR_ARG and launches nothing
    (the pointers are never dereferenced)."""
    lib = nv.lib()

    def desc(**over):
        d = nv.Sim2RealMonitorDesc()
        for n in nv.Sim2RealMonitorDesc.INPUTS + ("row",):
            setattr(d, n, 64)
        d.B, d.P, d.J, d.image_size = 4, 8, 7, 256.0
        for k, v in over.items():
            setattr(d, k, v)
        return d
    assert lib.hrp_sim2real_monitor(None, None) == -1
    for over, word in ((dict(B=0), b"B=0"), (dict(B=-3), b"B=-3"), (dict(J=25), b"J=25"), (dict(P=33), b"P=33"), (dict(J=0), b"J=0"),
                       (dict(rows=64, row_index=4, capacity=4), b"capacity"), (dict(rows=64, row_index=-1, capacity=4), b"capacity"),
                       (dict(rows=64, row_index=0, capacity=0), b"capacity"), (dict(row=None), b"null row")):
        assert lib.hrp_sim2real_monitor(C.byref(desc(**over)), None) == -1, over
        assert word in lib.hrp_last_error(), (over, lib.hrp_last_error())
    for n in nv.Sim2RealMonitorDesc.INPUTS:
        assert lib.hrp_sim2real_monitor(C.byref(desc(**{n: None})), None) == -1, n
        assert b"null" in lib.hrp_last_error(), n
    with pytest.raises(nv.HrpError, match="sim2real_monitor"):
        nv.call("hrp_sim2real_monitor", C.byref(desc(B=0)), None)


# ---- 4. what the step refuses ---------------------------------------------------------------------------------------------------

class Args(dict):
    __getattr__ = dict.__getitem__


def step_args(**over):
    a = Args(urdf_robot_name="panda", use_origin_bbox=False, use_extended_bbox=True, reference_keypoint_id=3,
             train_ds_names="dream/synthetic/panda_synth_train_dr", use_joint_valid_mask=False, known_joint=False,
             joint_individual_weights=None, image_size=256.0, pose_loss_func="mse", rot_loss_func="mse", trans_loss_func="l2norm",
             depth_loss_func="l1", uv_loss_func="l2norm", kp2d_loss_func="l2norm", kp3d_loss_func="l2norm", mask_loss_func="mse_mean",
             mask_loss_weight=0.0, iou_loss_weight=1.0, scale_loss_weight=0.0, align_3d_loss_weight=1.0,
             use_rootnet_with_reg_int_shared_backbone=True, use_rootnet_with_reg_with_int_separate_backbone=False)
    a.update(over)
    return a


def make_batch(B, seed, image_ids=None, hw=(480, 640)):
    """A batch in the reference's schema (host tensors) around ``make_case``'s ground truth for the panda."""
    from hrpe_amd.lib.dataset.const import JOINT_NAMES
    pred, gt, K, _ = make_case(B, 8, 7, seed, mask="zeros")
    g = torch.Generator().manual_seed(seed + 1)
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    R = R * torch.sign(torch.linalg.det(R)).reshape(B, 1, 1)
    TCO = torch.eye(4).repeat(B, 1, 1)
    TCO[:, :3, :3], TCO[:, :3, 3] = R, gt["kp3d"][:, 0]
    K_original = torch.tensor([[560.0, 0, 320.0], [0, 560.0, 240.0], [0, 0, 1.0]]).repeat(B, 1, 1)
    h = torch.einsum("bij,bkj->bki", K_original, gt["kp3d"])
    bbox = torch.tensor([[20.0, 30.0, 220.0, 200.0]]).repeat(B, 1)
    img = torch.randint(0, 256, (B, 3, 8, 8), generator=g, dtype=torch.uint8)
    return {"root": {"images": img, "K": K, "bbox_strict_bounded": bbox, "bbox_gt2d_extended": bbox},
            "other": {"images": img, "K": K, "keypoints_2d": gt["kp2d"], "valid_mask_crop": gt["mask"], "keypoints_3d": gt["kp3d"]},
            "TCO": TCO, "K_original": K_original, "keypoints_2d_original": h[..., :2] / h[..., 2:3], "valid_mask": gt["mask"],
            "image_id": torch.arange(B) + 100 if image_ids is None else torch.as_tensor(image_ids),
            "images_original": torch.randint(0, 256, (B, 3) + tuple(hw), generator=g, dtype=torch.uint8),
            "jointpose": {n: [float(gt["pose"][b, j]) for b in range(B)] for j, n in enumerate(JOINT_NAMES["panda"])}}


class FiveTuple(torch.nn.Module):
    def forward(self, reg_images, root_images, k_values, K=None):
        B = reg_images.shape[0]
        return torch.zeros(B, 8), torch.zeros(B, 6), torch.zeros(B, 3), torch.zeros(B, 2), torch.zeros(B, 1)


def test_unsupported_options_raise_not_implemented():
    from hrpe_amd.lib.core import sim2real as S
    from hrpe_amd.lib.dataset.const import LINK_NAMES
    robot = types.SimpleNamespace(robot_type="panda", link_names=LINK_NAMES["panda"], dof=8)
    batch = make_batch(2, seed=1)
    # the option pair that selects the reference's 5-tuple model (:239-251), and a model that returns five values whatever the options say
    with pytest.raises(NotImplementedError, match="use_rootnet_with_reg_int_shared_backbone"):
        S.farward_loss(step_args(use_rootnet_with_reg_int_shared_backbone=False), batch, "cpu", FiveTuple(), robot, None)
    with pytest.raises(NotImplementedError, match="5-tuple"):
        S.farward_loss(step_args(reference_keypoint_id=0), batch, "cpu", FiveTuple(), robot, None)
    # a loss function outside the shipped ones, named
    for name, value in (("uv_loss_func", "mse"), ("trans_loss_func", "smoothl1"), ("pose_loss_func", "l1"), ("kp3d_loss_func", "l1"),
                        ("mask_loss_func", "dice")):
        with pytest.raises(NotImplementedError, match=name):
            S.farward_loss(step_args(**{name: value}), batch, "cpu", FiveTuple(), robot, None)
    for func in ("mse_mean", "bce", "mse_sum"):
        S.check_sim2real_options(step_args(mask_loss_func=func))
