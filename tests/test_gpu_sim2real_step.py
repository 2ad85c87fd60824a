"""The self-supervised trainer's step on the device: hrp_sim2real_monitor (csrc/sim2real_step.hip), TrainMeters, farward_loss,
Sim2RealEvaluator and validate (lib/core/sim2real.py).

Reference and bound.  No fixture can come from the reference (its step is a closure inside scripts/train_sim2real.py and needs
pytorch3d, cv2 and CUDA): the kernel is held to the float64 restatement of :313-400 in tests/test_sim2real_step_host.py
(``reference_row``), every term within rtol 2e-5 - the project's tolerance for hrp_pose_loss terms (golden_pose_loss.npz test).  The
seeded cases (``make_case`` there) keep that a statement about the arithmetic: errors of centimetres on metres and of tens of
pixels on coordinates of hundreds, and a mean translation error far from the 0.5 switch on either side.  Sums: at most 65 * 15
terms, added per sample and then over the samples in fp32 - about sqrt(n) * 6e-8 relative.  Everything that is the same launches
(the copied mask terms, repeats, the meters' fp64 sums, the step against its hand-composed form, validate against
function.Evaluator) is compared bit for bit."""
import math

import numpy as np
import pytest
import torch

from test_sim2real_step_host import COMPUTED, ROW, RTOL, check_row, make_batch, make_case, reference_row, step_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def robot_of(robot_type):
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    return URDFRobot(robot_type)


def to_dev(case):
    pred, gt, K, size = case
    return tuple(t.to(DEV) for t in pred), {k: v.to(DEV) for k, v in gt.items()}, K.to(DEV), size


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. the kernel against the float64 restatement ------------------------------------------------------------------------------

@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
@pytest.mark.parametrize("robot_type", ["panda", "baxter"])
@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_monitor_kernel_matches_float64_restatement(B, robot_type, far):
    """One sample, an odd count, a full wave (one chunk of the kernel) and one more; the panda (P 8, J 7) and the robot with the
    widest tables (baxter: P 15, J 17); the mean translation error on each side of 0.5; a mask with zeros and one image masked out
    entirely; an all-zero mask for the whole batch (NaN in loss_error2d, the other terms finite)."""
    from hrpe_amd import _native as nv
    from hrpe_amd.lib.core import sim2real as S
    robot = robot_of(robot_type)
    P, J = robot.dof, robot.nkp
    assert (P, J) == ((8, 7) if robot_type == "panda" else (15, 17)) and J <= nv.FK_MAX_KP and P <= nv.FK_MAX_JOINTS
    mt = torch.tensor([0.4375, 0.03125, 0.71875, 1.625, 0.0859375], device=DEV)
    for mask in ("zeros", "none"):
        case = make_case(B, P, J, seed=1000 * B + J + (1 if far else 0), far=far, mask=mask)
        pred, gt, K, size = to_dev(case)
        ref = reference_row(*case, mt)
        e = float(torch.norm(case[0][2] - case[1]["root_trans"], dim=1).mean())
        assert (e > 0.55) == far and (far or e < 0.1)
        if mask == "zeros":
            assert float(gt["mask"].min()) == 0.0 and float(gt["mask"].max()) == 1.0 and (B == 1 or float(gt["mask"][0].max()) == 0.0)
        row, terms = S.sim2real_monitor(pred, gt, K, size, mask_terms=mt)
        assert row.is_cuda and row.shape == (12,) and not row.requires_grad and tuple(terms) == ROW
        check_row(row, ref, f"B={B} {robot_type} {'far' if far else 'near'} mask={mask}: ")
        assert math.isnan(float(row[6])) == (mask == "none")
        assert all(math.isfinite(float(row[i])) for i in range(12) if i != 6)
        # the copied entries: the bits of mask_terms, in the row's order; zero without them
        assert torch.equal(bits(row[[0, 8, 9, 10, 11]]), bits(mt[[0, 1, 3, 2, 4]]))
        row0, _ = S.sim2real_monitor(pred, gt, K, size)
        assert torch.equal(bits(row0[[0, 8, 9, 10, 11]]), torch.zeros(5, dtype=torch.int32))
        assert torch.equal(bits(row0[1:8]), bits(row[1:8]))


def test_monitor_python_side_rejects_wrong_shapes_and_capacity():
    from hrpe_amd import _native as nv
    from hrpe_amd.lib.core import sim2real as S
    pred, gt, K, size = to_dev(make_case(3, 8, 7, seed=3))
    rows = torch.full((2, 12), -1.0, device=DEV)
    with pytest.raises(nv.HrpError, match="capacity"):
        S.sim2real_monitor(pred, gt, K, size, rows=rows, row_index=2)
    with pytest.raises(nv.HrpError, match="gt_kp2d"):
        S.sim2real_monitor(pred, dict(gt, kp2d=gt["kp2d"][:, :6]), K, size)
    with pytest.raises(nv.HrpError, match="mask_terms"):
        S.sim2real_monitor(pred, gt, K, size, mask_terms=torch.zeros(4, device=DEV))
    torch.cuda.synchronize()
    assert float(rows.max()) == -1.0
    row, _ = S.sim2real_monitor(pred, gt, K, size, rows=rows, row_index=1)
    assert torch.equal(bits(rows[1]), bits(row)) and float(rows[0].max()) == -1.0


# ---- 2. reproducibility and the meters ------------------------------------------------------------------------------------------

def test_repeats_are_bit_equal_and_meters_hold_the_float64_running_sum():
    from hrpe_amd.lib.core import sim2real as S
    pred, gt, K, size = to_dev(make_case(65, 15, 17, seed=21, far=True))
    a, _ = S.sim2real_monitor(pred, gt, K, size)
    b, _ = S.sim2real_monitor(pred, gt, K, size)
    assert torch.equal(bits(a), bits(b))
    meters = S.TrainMeters(DEV)
    acc, rows = np.zeros(12, np.float64), []
    for i in range(5):
        pred, gt, K, size = to_dev(make_case(3 + i, 8, 7, seed=30 + i, far=i % 2 == 1, mask="ones"))
        row, _ = S.sim2real_monitor(pred, gt, K, size, mask_terms=torch.rand(5, device=DEV), meters=meters)
        rows.append(row)
    for row in rows:                                      # the float64 running sum of the five rows, in order
        acc = acc + row.cpu().double().numpy()
    assert np.array_equal(meters.sum.cpu().numpy(), acc) and int(meters.count) == 5
    means = meters.read_and_reset()
    assert tuple(means) == ROW and [means[k] for k in ROW] == list(acc / 5)
    assert float(meters.sum.abs().max()) == 0.0 and int(meters.count) == 0
    S.sim2real_monitor(pred, gt, K, size, meters=meters)
    assert int(meters.count) == 1


# ---- 3. graph capture and replay ------------------------------------------------------------------------------------------------

def test_monitor_launch_is_graph_capturable():
    """The monitor launch alone in a captured graph (a single serial node), replayed twice with the inputs overwritten in between:
    the rows follow the inputs and the meters' count advances by one per replay."""
    from hrpe_amd.lib.core import sim2real as S
    cases = [to_dev(make_case(5, 8, 7, seed=50 + i, far=i == 1)) for i in range(3)]
    pred = tuple(t.clone() for t in cases[0][0])
    gt = {k: v.clone() for k, v in cases[0][1].items()}
    K, size = cases[0][2].clone(), cases[0][3]
    mt = torch.rand(5, device=DEV)
    meters = S.TrainMeters(DEV)
    eager = [S.sim2real_monitor(c[0], c[1], c[2], size, mask_terms=mt)[0].clone() for c in cases]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        row, _ = S.sim2real_monitor(pred, gt, K, size, mask_terms=mt, meters=meters)
    torch.cuda.synchronize()
    assert int(meters.count) == 0                          # capturing launches nothing
    for n, c in enumerate(cases[1:], start=1):
        for dst, src in zip(pred, c[0]):
            dst.copy_(src)
        for k in gt:
            gt[k].copy_(c[1][k])
        K.copy_(c[2])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(row), bits(eager[n])) and int(meters.count) == n
    assert not torch.equal(bits(eager[1]), bits(eager[2]))


# ---- 4. farward_loss(train=True) ------------------------------------------------------------------------------------------------

def test_farward_loss_train_is_the_hand_composed_step_plus_one_monitor_launch():
    """B = 2, the synthetic box mesh and the 60 x 80 renderer of tests/test_gpu_silhouette.py's end-to-end test (a soft band, so
    that the IoU term has a gradient), seg_net a callable that returns masks rendered from a perturbed pose.  loss and every
    parameter gradient bit-equal to the step composed by hand from prepare_batch, get_rendered_masks and sim2real_mask_loss (the
    same launches); loss_dict: the eleven names, no gradient, the seven monitor terms within 2e-5 of float64 on the model's own
    predictions, the four mask terms the bits of sim2real_mask_loss's; every BatchNorm in eval(); one renderer for both calls."""
    from hrpe_amd.lib.core import function as F
    from hrpe_amd.lib.core import sim2real as S
    from synth import synth_inputs
    from test_gpu_silhouette import box_mesh
    import test_gpu_model as M
    m = M.build_full().train()
    B = 2
    x_reg, x_root, kv, Kc = synth_inputs(B)
    batch = make_batch(B, seed=77)
    side = torch.sqrt(Kc[:, 0, 0] * Kc[:, 1, 1] * 1e6) / kv              # the bounding box whose k_value is synth_inputs'
    bbox = torch.stack([torch.zeros(B), torch.zeros(B), side, side], 1)
    batch["root"].update(images=x_root * 255.0, K=Kc, bbox_strict_bounded=bbox, bbox_gt2d_extended=bbox)
    batch["other"].update(images=x_reg * 255.0, K=Kc)
    args = step_args(mask_loss_weight=1.0)
    weights = dict(mask=1.0, iou=1.0, scale=0.0, align=1.0)
    renderer = S.renderer_for(m.robot, batch["K_original"][0], DEV, mesh=box_mesh(11), scale=0.125, sigma=1e-4)
    assert renderer.image_size == (60, 80) and renderer.sigma == 1e-4
    p = F.prepare_batch(batch, m.robot, DEV, reference_keypoint_id=3)
    with torch.no_grad():
        pose, rot, trans = m(p["reg_images"], p["root_images"], p["k_values"], K=p["other_K"])[:3]
        seg = m.robot.get_rendered_masks(pose, rot, trans + torch.tensor([0.02, -0.01, 0.03], device=DEV), renderer, root=3)
    assert float(seg.sum()) > 0
    seen = []

    def seg_net(images_255):
        assert images_255.shape == (B, 3, 480, 640) and images_255.dtype == torch.float32 and images_255.is_cuda
        assert torch.equal(images_255.cpu(), batch["images_original"].float())
        seen.append(1)
        return seg[:, None]

    # the step composed by hand
    for mod in m.modules():
        if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
            mod.eval()
    pred = m(p["reg_images"], p["root_images"], p["k_values"], K=p["other_K"])
    rendered = m.robot.get_rendered_masks(pred[0], pred[1], pred[2], renderer, root=3)
    loss_h, terms_h = F.sim2real_mask_loss(rendered, seg[:, None], pred[7], pred[6], "mse_mean", weights)
    loss_h.backward()
    grads_h = {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}
    assert len(grads_h) > 100 and any(float(g.abs().max()) > 0 for g in grads_h.values())
    for q in m.parameters():
        q.grad = None
    # the library's step
    m.train()                                              # (puts every BatchNorm back in training mode: farward_loss must undo it)
    meters = S.TrainMeters(DEV)
    outs = []
    hook = m.register_forward_hook(lambda mod, inp, out: outs.append(tuple(t.detach().clone() for t in out)))
    loss, loss_dict = S.farward_loss(args, batch, DEV, m, m.robot, seg_net, train=True, meters=meters)
    hook.remove()
    loss.backward()
    assert seen == [1] and torch.equal(bits(loss), bits(loss_h)) and loss.requires_grad
    grads = {n: q.grad for n, q in m.named_parameters() if q.grad is not None}
    assert set(grads) == set(grads_h)
    bad = [n for n in grads if not torch.equal(bits(grads[n]), bits(grads_h[n]))]
    assert not bad, bad[:8]
    assert tuple(loss_dict) == S.LOSS_KEYS and len(loss_dict) == 11
    assert all(v.is_cuda and not v.requires_grad and v.shape == () for v in loss_dict.values())
    ref = reference_row(outs[0], p["gt"], p["other_K"], 256.0)
    for k in COMPUTED:
        print(f"{k}: {float(loss_dict[k])!r} vs {ref[k]!r}")
        np.testing.assert_allclose(float(loss_dict[k]), ref[k], rtol=RTOL, err_msg=k)
    for k in ("loss_mask", "loss_iou", "loss_scale", "loss_error3d_align"):
        assert torch.equal(bits(loss_dict[k]), bits(terms_h[k])), k
    assert m.training and all(not mod.training for mod in m.modules() if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)))
    means, n = meters.read()
    assert n == 1 and means["loss"] == float(loss.detach()) and means["loss_joint"] == float(loss_dict["loss_joint"])
    # a second call finds the same renderer (the reference rebuilds it, and reloads every .obj, per step)
    for q in m.parameters():
        q.grad = None
    loss2, _ = S.farward_loss(args, batch, DEV, m, m.robot, seg_net, train=True, meters=meters)
    assert S.renderer_for(m.robot, batch["K_original"][0], DEV) is renderer and len(m.robot._sim2real_renderers) == 1
    assert torch.equal(bits(loss2), bits(loss)) and int(meters.count) == 2
    # known_joint (:404-405): the mesh is posed with the ground-truth joints, loss_joint vanishes
    _, d3 = S.farward_loss(step_args(mask_loss_weight=1.0, known_joint=True), batch, DEV, m, m.robot, seg_net, train=True)
    assert float(d3["loss_joint"]) == 0.0 and not torch.equal(bits(d3["loss_iou"]), bits(loss_dict["loss_iou"]))


# ---- 5. validate ----------------------------------------------------------------------------------------------------------------

NAMES8 = ["pose", "rot", "trans", "root_uv", "depth", "uvd", "xyz_int", "xyz_fk"]


class Stub(torch.nn.Module):
    def __init__(self, preds):
        super().__init__()
        self.preds, self.calls = preds, 0

    def forward(self, reg_images, root_images, k_values, K=None):
        out = self.preds[self.calls % len(self.preds)]
        self.calls += 1
        return tuple(t.clone() for t in out)


class Recorder:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, epoch):
        assert tag not in self.scalars and isinstance(value, float), tag
        self.scalars[tag] = (value, epoch)


@pytest.fixture(scope="module")
def val_setup():
    """Batches of 2, 2 and 1 images (the last one ragged) in the reference's schema, image ids out of order, and the predictions a
    stub model returns for them."""
    ids = [[17, 3], [40, 8], [25]]
    loader = [make_batch(len(i), seed=200 + n, image_ids=i, hw=(8, 8)) for n, i in enumerate(ids)]
    preds = []
    for n, b in enumerate(loader):
        pred = to_dev(make_case(len(ids[n]), 8, 7, seed=300 + n, mask="ones"))[0]
        kp3d = b["other"]["keypoints_3d"].to(DEV)
        g = torch.Generator().manual_seed(400 + n)
        noise = lambda *sh: (0.05 * torch.randn(*sh, generator=g)).to(DEV)   # noqa: E731
        preds.append(pred[:6] + (kp3d + noise(*kp3d.shape), kp3d + noise(*kp3d.shape)))
    return loader, preds, robot_of("panda"), sum(ids, [])


def test_validate_matches_function_evaluator_and_the_monitor_rows(val_setup):
    from hrpe_amd.lib.core import function as F
    from hrpe_amd.lib.core import sim2real as S
    loader, preds, robot, ids = val_setup
    args = step_args()
    model, writer = Stub(preds).train(), Recorder()
    auc, loss_mean = S.validate(args, 7, "dr", loader, model, robot, None, writer, DEV, epoch=6)
    assert model.training and model.calls == 3
    # the same predictions through function.Evaluator, batch by batch, and through the monitor
    ev, rows = F.Evaluator(robot, 5, reference_keypoint_id=3, device=DEV), []
    for b, pr in zip(loader, preds):
        p = F.prepare_batch(b, robot, DEV, reference_keypoint_id=3)
        fk = robot.get_keypoints_root(pr[0], pr[1], pr[2], root=3)
        ev.add(dict(kp3d_fk=fk, kp3d_int=pr[6], joint=pr[0], rot=pr[1]),
               dict(kp3d=p["gt"]["kp3d"], kp2d_original=b["keypoints_2d_original"], K_original=b["K_original"], joint=p["gt"]["pose"],
                    rot=p["gt"]["rot"]))
        row, _ = S.sim2real_monitor(pr, p["gt"], p["other_K"], 256.0)
        check_row(row, reference_row(pr, p["gt"], p["other_K"], 256.0))
        rows.append(row.cpu().double().numpy())
    s = ev.summary()
    mean = (rows[0] + rows[1] + rows[2]) / 3
    want = {"Val/loss": 0.0, "Val/mask_loss": 0.0, "Val/scale_loss": 0.0, "Val/align_loss": 0.0, "Val/iou_loss": 0.0,
            "Val/pose_loss": mean[1], "Val/rot_loss": mean[2], "Val/trans_loss": mean[3], "Val/uv_loss": mean[4], "Val/depth_loss": mean[5],
            "Val/error2d_loss": mean[6], "Val/error3d_loss": mean[7], "Val/mean_joint_error": s["mean_joint_error"],
            "Val/AUC_ADD": s["ADD/AUC"], "Val/AUC_PCK": s["PCK/AUC"], "Val/AUC_ADD_integral_xyz_metrics": s["integral"]["ADD/AUC"],
            "Val/AUC_PCK_integral_xyz_metrics": s["integral"]["PCK/AUC"]}
    for th in F.ADD_THRESHOLDS:
        want[f"Val/ADD_{th}_mm"] = s[f"ADD_{th}_mm"]
    for th in F.PCK_THRESHOLDS:
        want[f"Val/PCK_{th}_pixel"] = s[f"PCK_{th}_pixel"]
    for k in range(7):
        want[f"Val/distance3D_keypoint_{k + 1}"] = s["meters"]["dis3d"][k]
        want[f"Val/distance2D_keypoint_{k + 1}"] = s["meters"]["dis2d"][k]
    for k in range(8):
        want[f"Val/l1error_joint_{k + 1}"] = s["meters"]["l1_joint"][k]
    assert len(want) == 17 + 16 + 14 + 8 and set(writer.scalars) == {t + "_dr" for t in want}
    for tag, v in want.items():
        got, epoch = writer.scalars[tag + "_dr"]
        assert got == float(v) or (math.isnan(got) and math.isnan(float(v))), (tag, got, v)
        assert epoch == (6 if tag.endswith("_integral_xyz_metrics") else 7), tag       # :612-613 log at the epoch loop's variable
    assert auc == s["ADD/AUC"] and loss_mean == 0.0 and isinstance(auc, float)
    # without a writer and without `epoch`
    assert S.validate(args, 7, "dr", loader, Stub(preds), robot, None, None, DEV) == (auc, 0.0)
    # the evaluator itself: image ids in loader order, the rows, the worst cases
    sev = S.Sim2RealEvaluator(robot, 2, reference_keypoint_id=3, device=DEV, batch_capacity=1)      # (grows twice on the way)
    model = Stub(preds)
    with torch.no_grad():
        for b in loader:
            loss, loss_dict, md = S.farward_loss(args, b, DEV, model, robot, None, train=False, evaluator=sev)
            assert float(loss) == 0.0 and tuple(loss_dict) == S.LOSS_KEYS and md["idx"].is_cuda and set(F.METRIC_KEYS) < set(md)
    assert (sev.count, sev.batches) == (5, 3)
    ss = sev.summary()
    assert list(ss["image_ids"]) == ids
    assert np.array_equal(sev.rows[:3].cpu().double().numpy(), np.stack(rows))
    assert [ss["meters"][k] for k in ROW] == [float(v) for v in mean]
    assert np.array_equal(ss["meters"]["dis3d"], s["meters"]["dis3d"]) and ss["ADD/AUC"] == s["ADD/AUC"]
    dis = ev.per_image[0, :5].cpu().numpy()
    assert ss["worst_cases"] == S.worst_cases(dis, np.asarray(ids)) == sev.worst_cases()
    # get_lowest: the cut worst-case list of the host formula - five images, position 0 only: the worst image
    view_ids, errors = S.validate(args, 0, "dr", loader, Stub(preds), robot, None, None, DEV, get_lowest=True)
    assert (view_ids, errors) == S.worst_cases(dis, np.asarray(ids)) == ([ids[int(dis.argmax())]], [float(dis.max())])
    with pytest.raises(AssertionError):
        S.validate(args, 0, "orb", loader, Stub(preds), robot, None, None, DEV, get_lowest=True)     # :537-539


def test_farward_loss_eval_without_an_evaluator(val_setup):
    from hrpe_amd.lib.core import sim2real as S
    loader, preds, robot, ids = val_setup
    with torch.no_grad():
        loss, loss_dict, md = S.farward_loss(step_args(), loader[2], DEV, Stub(preds[2:]), robot, None, train=False)
    assert float(loss) == 0.0 and md["image_dis3d_avg"].shape == (1,) and md["idx"].tolist() == [25]
    ref = reference_row(preds[2], {k: v for k, v in _gt(loader[2], robot).items()}, loader[2]["other"]["K"], 256.0)
    for k in COMPUTED:
        np.testing.assert_allclose(float(loss_dict[k]), ref[k], rtol=RTOL, err_msg=k)
    assert all(float(loss_dict[k]) == 0.0 for k in ("loss_mask", "loss_scale", "loss_iou", "loss_error3d_align"))


def _gt(batch, robot):
    from hrpe_amd.lib.core.function import prepare_batch
    return prepare_batch(batch, robot, DEV, reference_keypoint_id=3)["gt"]
