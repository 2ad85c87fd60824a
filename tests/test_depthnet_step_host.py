"""Host-side checks of the DepthNet trainer's step (hrpe_amd.lib.core.depthnet) against the fixture the reference's own trainer wrote
(tests/golden/golden_depthnet_step.npz, gen_golden_depthnet_step.py); no GPU needed.

Tolerances.  Losses and gradients: rtol 2e-5, the project's tolerance for fixture loss terms (header of test_gpu_eval.py).  Per-image
errors: atol 2.4e-7 = 2 ulp of fp32 in [1, 2), the fixture's depth range; with the reference's division by 1000 they are expected
bit-equal.  k_values: 2 ulp (rtol 2^-22) - the same fp32 operations in the same order, every one correctly rounded.  The summary's
rootz_loss is the same fp64 sum (rtol 1e-12); the three error means are fp32 means over 11 values on both sides, compared at
rtol 1e-6 (above (n - 1) * 2^-24, the bound of an fp32 sum of n values in any order)."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import depthnet_step_fixture as fx
from conftest import ROOT
from hrpe_amd import _native as nv
from hrpe_amd.lib.core import depthnet as dn

PARTS = [(part, i) for part in ("train", "val") for i in range(3)]


@pytest.mark.parametrize("run", list(fx.RUNS))
def test_host_loss_gradient_and_errors_match_the_reference(run):
    G, o = fx.golden(), fx.run_options(run)
    for part, i in PARTS:
        pred = fx.pred_of(run, part, i).requires_grad_(part == "train")
        gt = fx.gt_of(run, part, i)
        ev = dn.DepthEvaluator(1, device="cpu", batch_capacity=1) if part == "val" else None
        loss = dn.depthnet_loss(pred, gt, evaluator=ev, **o)
        np.testing.assert_allclose(loss.item(), G[f"{run}:{part}{i}:loss"], rtol=fx.LOSS_RTOL, atol=0)
        if part == "train":
            loss.backward()
            np.testing.assert_allclose(pred.grad.numpy(), G[f"{run}:{part}{i}:dpred"], rtol=fx.LOSS_RTOL, atol=0)
        else:
            for e, name in zip(ev.last_errors(), dn.DepthEvaluator.ROWS):
                np.testing.assert_allclose(e.numpy(), G[f"{run}:{part}{i}:{name}"], rtol=0, atol=fx.ERROR_ATOL)


def test_sign_of_zero_is_pinned_by_the_fixture():
    """xy runs, training batch 0: sample 1 predicts x exactly, sample 0 has mask 0 - the l1 gradient there is 0, not +-1 / n."""
    G = fx.golden()
    gt = fx.gt_of("xy_l1", "train", 0)
    assert G["xy_l1:train0:pred"][1, 0] == gt["root_trans"][1, 0].item() and gt["mask"].tolist() == [0.0, 1.0, 1.0, 1.0]
    d = G["xy_l1:train0:dpred"]
    assert d[1, 0] == 0.0 and d[1, 1] != 0.0 and not d[0, 0:2].any() and d[0, 2] != 0.0


@pytest.mark.parametrize("run", list(fx.RUNS))
def test_prepare_depthnet_batch(run):
    """k_values (abs with the negative fx of train1 / val2; the bbox and intrinsics each run's options select), the root view's
    ground truth, uint8 images kept."""
    import types
    G, args = fx.golden(), fx.run_args(run)
    robot = types.SimpleNamespace(robot_type="kuka", link_names=["l"] * 8)
    assert G["train1:K"][1, 0, 0] < 0 and G["val2:K"][1, 0, 0] < 0
    for part, i in PARTS:
        batch = fx.batch_of(part, i)
        p = dn.prepare_depthnet_batch(batch, robot, "cpu", args.reference_keypoint_id, args.use_origin_bbox, args.use_extended_bbox,
                                      args.multi_kp, args.kps_need_depth)
        assert p["images"].dtype == torch.uint8 and torch.equal(p["images"], batch["root"]["images"])
        assert p["k_values"].dtype == torch.float32 and torch.isfinite(p["k_values"]).all()
        np.testing.assert_allclose(p["k_values"].numpy(), G[f"{run}:{part}{i}:k_values"], rtol=2.0 ** -22, atol=0)
        want = fx.gt_of(run, part, i)
        for k in ("root_trans", "kp3d", "mask"):
            assert torch.equal(p["gt"][k], want[k]), k
        assert torch.equal(p["gt"]["root_depth"], want["root_trans"][:, 2:3])
        if args.multi_kp:
            assert torch.equal(p["gt"]["kp_depths"], want["kp3d"][:, [1, 3, 5], 2])
    batch["root"]["images"] = batch["root"]["images"].float()          # the reference's loaders: float tensors holding 0..255
    p = dn.prepare_depthnet_batch(batch, robot, "cpu", args.reference_keypoint_id, args.use_origin_bbox, args.use_extended_bbox)
    assert p["images"].dtype == torch.float32 and torch.equal(p["images"], batch["root"]["images"] / 255.)


def check_summary(s, run, loss_rtol):
    G = fx.golden()
    np.testing.assert_allclose(s["rootz_loss"], G[f"{run}:scalar:Val/rootz_loss_dr"], rtol=loss_rtol, atol=0)
    for tag in fx.VAL_TAGS[1:]:
        np.testing.assert_allclose(s[tag], G[f"{run}:scalar:Val/{tag}_dr"], rtol=1e-6, atol=0)


@pytest.mark.parametrize("run", ["l1", "xy_mse"])
def test_depth_evaluator_summary_arithmetic(run):
    """The recorded per-batch losses and per-image errors through the accumulators (capacity 8 and 2: both grow once)."""
    G = fx.golden()
    ev = dn.DepthEvaluator(8, device="cpu", batch_capacity=2)
    for i, B in enumerate(fx.sizes()):
        ev.add_host(torch.tensor(G[f"{run}:val{i}:loss"]), *[torch.tensor(G[f"{run}:val{i}:{n}"]) for n in ev.ROWS])
        assert ev.last == (sum(fx.sizes()[:i]), B, i)
    assert (ev.count, ev.batches, ev.capacity, ev.batch_capacity) == (11, 3, 16, 4)
    assert not ev.errors[:, 11:].any() and not ev.losses[3:].any()
    check_summary(ev.summary(), run, 1e-12)


@pytest.mark.parametrize("run", list(fx.RUNS))
def test_validate_on_the_host_logs_the_reference_scalars(run):
    G, args = fx.golden(), fx.run_args(run)
    loader = [fx.batch_of("val", i) for i in range(3)]
    model, writer = fx.StubModel([fx.pred_of(run, "val", i) for i in range(3)]), fx.Recorder()
    model.train()
    ret = dn.validate(args, 7, "dr", loader, model, writer, "cpu")
    assert model.training and model.calls == 3
    assert sorted(writer.scalars) == sorted(f"Val/{t}_dr" for t in fx.VAL_TAGS) and all(e == 7 for _, e in writer.scalars.values())
    check_summary({t: writer.scalars[f"Val/{t}_dr"][0] for t in fx.VAL_TAGS}, run, fx.LOSS_RTOL)
    np.testing.assert_allclose(ret, G[f"{run}:validate_return"], rtol=1e-6, atol=0)
    assert ret == writer.scalars["Val/mean_depth_error_dr"][0]
    for i in range(3):
        np.testing.assert_allclose(model.k_values[i].numpy(), G[f"{run}:val{i}:k_values"], rtol=2.0 ** -22, atol=0)


def test_farward_loss_returns_what_the_reference_returns():
    args = fx.run_args("xy_l1")
    model = fx.StubModel([fx.pred_of("xy_l1", "val", 2)])
    loss = dn.farward_loss(args, fx.batch_of("val", 2), "cpu", model, train=True)
    assert loss.shape == () and model.training
    out = dn.farward_loss(args, fx.batch_of("val", 2), "cpu", model, train=False)
    assert len(out) == 4 and not model.training and all(e.shape == (3,) for e in out[1:])
    assert out[0].item() == loss.item()


def test_depth_loss_desc_size_matches_c():
    prog = ('#include <stdio.h>\n#include "hrp.h"\nint main(void) { printf("%zu %d\\n", sizeof(hrp_depth_loss_desc), '
            'HRP_DEPTH_LOSS_MAX_KP); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "s.c"), "w") as fh:
            fh.write(prog)
        exe = os.path.join(td, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe], check=True)
        size, max_kp = [int(v) for v in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert size == C.sizeof(nv.DepthLossDesc) and max_kp == nv.DEPTH_LOSS_MAX_KP == 16
    assert [n for n, _ in nv.DepthLossDesc._fields_[:8]] == list(nv.DepthLossDesc.POINTERS)
    assert nv.DEPTH_LOSS_KINDS == {"l1": 0, "mse": 1} and nv.XY_LOSS_KINDS == {None: 0, "l1": 1, "mse": 2}


def test_depth_loss_rejects_bad_descriptors_without_a_gpu():
    """Every rejection is HRP_ERR_ARG with a text naming it, before anything launches (the pointers are never dereferenced)."""
    lib = nv.lib()

    def desc(**over):
        d = nv.DepthLossDesc()
        for n in nv.DepthLossDesc.POINTERS:
            setattr(d, n, 64)
        d.B, d.W, d.J, d.capacity, d.batch_capacity, d.want_grad = 4, 1, 8, 16, 2, 1
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def rejected(text, **over):
        d = desc(**over)
        rc = lib.hrp_depth_loss(C.byref(d), None)
        assert rc == -1 and text in lib.hrp_last_error(), (over, rc, lib.hrp_last_error())

    assert lib.hrp_depth_loss(None, None) == -1 and b"null descriptor" in lib.hrp_last_error()
    rejected(b"null pred", pred=None)
    rejected(b"B=0", B=0)
    rejected(b"B=-3", B=-3)
    rejected(b"W=3", W=3)                                                  # plain mode with three columns
    rejected(b"W=1", xy_loss=1, root_col=0)                                # the xy branch has three
    rejected(b"W=3", nk=2, W=3, root_col=0)                                # multi_kp: W is nk
    rejected(b"root_col=1", root_col=1)
    rejected(b"root_col=3", nk=3, W=3, root_col=3)
    rejected(b"root_col=0", xy_loss=2, W=3, root_col=0)
    rejected(b"nk=17", nk=17, W=17)
    d = desc(nk=3, W=3, root_col=1)
    d.kp_index[0], d.kp_index[1], d.kp_index[2] = 1, 8, 5
    assert lib.hrp_depth_loss(C.byref(d), None) == -1 and b"kp_index[1]=8" in lib.hrp_last_error()
    rejected(b"null gt_kp3d", nk=1, W=1, gt_kp3d=None)
    rejected(b"null mask", xy_loss=1, W=3, root_col=2, mask=None)
    rejected(b"capacity", offset=13)
    rejected(b"batch 2", offset=12, batch_index=2)
    rejected(b"null losses", losses=None)
    rejected(b"unknown depth_loss kind 2", depth_loss=2)
    rejected(b"unknown xy_loss kind 3", xy_loss=3, W=3, root_col=2)
    rejected(b"exclude", xy_loss=1, nk=3, W=3, root_col=2)
    rejected(b"want_grad", d_pred=None)


def test_step_functions_keep_the_reference_signatures():
    p = list(inspect.signature(dn.farward_loss).parameters.values())
    assert [q.name for q in p[:5]] == ["args", "input_batch", "device", "model", "train"]
    assert p[4].default is True and all(q.default is not inspect.Parameter.empty for q in p[5:])
    assert list(inspect.signature(dn.validate).parameters) == ["args", "epoch", "dsname", "loader", "model", "writer", "device"]
    p = inspect.signature(dn.depthnet_loss).parameters
    assert list(p) == ["pred", "gt", "depth_loss_func", "xy_loss_func", "kps_need_depth", "reference_keypoint_id", "evaluator"]
    assert (p["depth_loss_func"].default, p["xy_loss_func"].default, p["reference_keypoint_id"].default) == ("l1", None, 3)
    assert list(inspect.signature(dn.prepare_depthnet_batch).parameters) == [
        "input_batch", "robot", "device", "reference_keypoint_id", "use_origin_bbox", "use_extended_bbox", "multi_kp", "kps_need_depth"]
    import hrpe_amd.lib.core.function as function          # the stage-2 module stays what it was
    assert "robot" in inspect.signature(function.farward_loss).parameters


@pytest.mark.parametrize("option", [dict(depth_loss_func="smoothl1"), dict(use_rootnet_xy_branch=True, xy_loss_func="smoothl1"),
                                    dict(multi_kp=True, kps_need_depth=[1, 3, 5], depth_loss_func="l2norm")])
def test_unknown_loss_functions_raise_before_the_device_is_touched(option):
    """The model and the batch are None: an option the reference does not know is refused before either is used."""
    args = fx.Args(fx.run_args("l1"))
    args.update(option)
    with pytest.raises(NotImplementedError, match="loss_func"):
        dn.farward_loss(args, None, "cuda:0", None, train=False)
    pred, gt = torch.zeros(2, 1), dict(root_trans=torch.ones(2, 3))
    with pytest.raises(NotImplementedError):
        dn.depthnet_loss(pred, gt, depth_loss_func="huber")
    with pytest.raises(NotImplementedError):
        dn.depthnet_loss(torch.zeros(2, 3), dict(gt, mask=torch.ones(2)), xy_loss_func="huber")
