"""The DepthNet trainer's step on the device: hrp_depth_loss (csrc/depth_loss.hip), depthnet_loss, DepthEvaluator, farward_loss, validate.

Tolerances (those of test_depthnet_step_host.py).  Losses and gradients: rtol 2e-5, the project's tolerance for fixture loss terms.
Per-image errors: atol 2.4e-7 = 2 ulp of fp32 in [1, 2), the depth range of the fixture and of the random cases here; the kernel
divides by 1000.0f as the reference does, so they are expected bit-equal.  Gradients against the host expressions carry in addition
atol 2^-23 * max|e| / 1000 with e = p / 1000 - g: the xy branch's depth gradient is a sum over the B targets (the reference's [B]
against [B, 1] broadcast) that may cancel, and an fp32 sum of B terms of size <= 2 max|e|, divided by B * B * 1000, is off by at
most (B - 1) * 2^-24 * B * 2 max|e| / (B * B * 1000) whatever its order.  Summary means: rtol 1e-6 (fp32 means of 11 values)."""
import ctypes as C

import numpy as np
import pytest
import torch

import depthnet_step_fixture as fx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARTS = [(part, i) for part in ("train", "val") for i in range(3)]


def to_dev(gt):
    return {k: v.to(DEV) for k, v in gt.items()}


def report(name, got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    print(f"{name}: max |diff| {d.max():.3e}, max rel {np.max(d / np.maximum(np.abs(ref), 1e-30)):.3e} (values up to {np.abs(ref).max():.3e})")


@pytest.mark.parametrize("run", list(fx.RUNS))
def test_kernel_matches_the_reference_fixture(run):
    from hrpe_amd.lib.core import depthnet as dn
    G, o = fx.golden(), fx.run_options(run)
    for part, i in PARTS:
        pred = fx.pred_of(run, part, i, DEV).requires_grad_(part == "train")
        ev = dn.DepthEvaluator(1, device=DEV, batch_capacity=1) if part == "val" else None
        loss = dn.depthnet_loss(pred, to_dev(fx.gt_of(run, part, i)), evaluator=ev, **o)
        key = f"{run}:{part}{i}:"
        report(key + "loss", loss.item(), G[key + "loss"])
        np.testing.assert_allclose(loss.item(), G[key + "loss"], rtol=fx.LOSS_RTOL, atol=0)
        if part == "train":
            (3.0 * loss).backward()                       # the backward is one multiply by the incoming gradient
            report(key + "dpred", pred.grad.cpu().numpy() / 3.0, G[key + "dpred"])
            np.testing.assert_allclose(pred.grad.cpu().numpy() / 3.0, G[key + "dpred"], rtol=fx.LOSS_RTOL, atol=0)
        else:
            for e, name in zip(ev.last_errors(), dn.DepthEvaluator.ROWS):
                report(key + name, e.cpu().numpy(), G[key + name])
                np.testing.assert_allclose(e.cpu().numpy(), G[key + name], rtol=0, atol=fx.ERROR_ATOL)
            assert ev.losses[0].item() == loss.item()


def random_case(B, mode, seed):
    """Host tensors of one batch: depths in [0.5, 2) m, predictions 30 mm / 0.03 m off, every fifth row masked, one y predicted exactly."""
    g = torch.Generator().manual_seed(seed)
    J = 8
    kp3d = torch.rand(B, J, 3, generator=g) * 1.5 + 0.5
    kp3d[:, :, 0:2] -= 1.25
    root_trans = kp3d[:, 3].clone()
    mask = torch.ones(B)
    mask[::5] = 0.0
    if mode == "xy":
        pred = torch.cat([root_trans[:, 0:2] + 0.03 * torch.randn(B, 2, generator=g),
                          root_trans[:, 2:3] * 1000.0 + 30.0 * torch.randn(B, 1, generator=g)], 1)
        pred[B - 1, 1] = root_trans[B - 1, 1]
    elif mode == "mkp":
        pred = kp3d[:, [1, 3, 5], 2] * 1000.0 + 30.0 * torch.randn(B, 3, generator=g)
    else:
        pred = root_trans[:, 2:3] * 1000.0 + 30.0 * torch.randn(B, 1, generator=g)
    return pred.contiguous(), dict(root_trans=root_trans, kp3d=kp3d, mask=mask)


MODES = {"plain": dict(xy_loss_func=None, kps_need_depth=None), "xy": dict(xy_loss_func=None, kps_need_depth=None),
         "mkp": dict(xy_loss_func=None, kps_need_depth=[1, 3, 5])}


@pytest.mark.parametrize("B", [1, 3, 257])          # 257: the kernel walks the batch in chunks of 256 samples
@pytest.mark.parametrize("mode", ["plain", "xy", "mkp"])
@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_kernel_matches_the_host_expressions(B, mode, kind):
    from hrpe_amd.lib.core import depthnet as dn
    o = dict(MODES[mode], depth_loss_func=kind, reference_keypoint_id=3)
    if mode == "xy":
        o["xy_loss_func"] = kind
    pred, gt = random_case(B, mode, 100 * B + len(mode))
    ph = pred.clone().requires_grad_(True)
    ev_h = dn.DepthEvaluator(B, device="cpu", batch_capacity=1)
    want = dn.depthnet_loss(ph, gt, evaluator=ev_h, **o)
    want.backward()
    pd = pred.clone().to(DEV).requires_grad_(True)
    ev = dn.DepthEvaluator(B, device=DEV, batch_capacity=1)
    loss = dn.depthnet_loss(pd, to_dev(gt), evaluator=ev, **o)
    loss.backward()
    name = f"B{B} {mode} {kind} "
    report(name + "loss", loss.item(), want.item())
    np.testing.assert_allclose(loss.item(), want.item(), rtol=fx.LOSS_RTOL, atol=0)
    col = 2 if mode == "xy" else (1 if mode == "mkp" else 0)
    e_max = float((pred[:, col].reshape(1, B) / 1000.0 - gt["root_trans"][:, 2].reshape(B, 1)).abs().max()) if mode == "xy" else \
        float((pred / 1000.0 - (gt["kp3d"][:, [1, 3, 5], 2] if mode == "mkp" else gt["root_trans"][:, 2:3])).abs().max())
    report(name + "dpred", pd.grad.cpu().numpy(), ph.grad.numpy())
    np.testing.assert_allclose(pd.grad.cpu().numpy(), ph.grad.numpy(), rtol=fx.LOSS_RTOL, atol=2.0 ** -23 * e_max / 1000.0)
    for e, w, row in zip(ev.last_errors(), ev_h.last_errors(), dn.DepthEvaluator.ROWS):
        np.testing.assert_allclose(e.cpu().numpy(), w.numpy(), rtol=0, atol=fx.ERROR_ATOL, err_msg=row)
    if mode == "xy" and kind == "l1":
        assert pd.grad[B - 1, 1].item() == 0.0 and not pd.grad[0, 0:2].any()          # sign(0) = 0; mask 0
    # d_pred null: a prediction that needs no gradient gets none, and the same loss
    again = dn.depthnet_loss(pred.to(DEV), to_dev(gt), **o)
    assert not again.requires_grad and again.item() == loss.item()


@pytest.mark.parametrize("run", ["l1", "xy_mse", "mkp_mse"])
def test_accumulators_over_an_epoch(run):
    """4, 4 and 3 images at offsets 0, 4, 8 into a capacity of 8 (grows once, as the batch capacity of 2 does); the summary equals the
    scalars the reference logged; nothing outside [0, 11) / [0, 3) is written."""
    from hrpe_amd.lib.core import depthnet as dn
    G, o = fx.golden(), fx.run_options(run)
    grown, roomy = dn.DepthEvaluator(8, device=DEV, batch_capacity=2), dn.DepthEvaluator(16, device=DEV, batch_capacity=4)
    roomy.errors.fill_(-7.0)
    roomy.losses.fill_(-7.0)
    for ev in (grown, roomy):
        for i, B in enumerate(fx.sizes()):
            dn.depthnet_loss(fx.pred_of(run, "val", i, DEV), to_dev(fx.gt_of(run, "val", i)), evaluator=ev, **o)
            assert ev.last == (sum(fx.sizes()[:i]), B, i)
        assert (ev.count, ev.batches, ev.capacity, ev.batch_capacity) == (11, 3, 16, 4)
    assert not grown.errors[:, 11:].any() and not grown.losses[3:].any()
    assert (roomy.errors[:, 11:] == -7.0).all() and (roomy.losses[3:] == -7.0).all()
    assert torch.equal(grown.errors[:, :11], roomy.errors[:, :11]) and torch.equal(grown.losses[:3], roomy.losses[:3])
    s = grown.summary()
    for tag in fx.VAL_TAGS:
        report(f"{run} {tag}", s[tag], G[f"{run}:scalar:Val/{tag}_dr"])
    np.testing.assert_allclose(s["rootz_loss"], G[f"{run}:scalar:Val/rootz_loss_dr"], rtol=fx.LOSS_RTOL, atol=0)
    for tag in fx.VAL_TAGS[1:]:
        np.testing.assert_allclose(s[tag], G[f"{run}:scalar:Val/{tag}_dr"], rtol=1e-6, atol=0)


def launch(pred, gt, o, outs, offset, batch_index):
    """One hrp_depth_loss launch into preallocated outputs (loss [1], grad [B, W], errors [3, cap], losses [nb])."""
    from hrpe_amd import _native as nv
    loss, grad, errors, losses = outs
    d = nv.DepthLossDesc()
    d.pred, d.gt_root_trans, d.gt_kp3d, d.mask = pred.data_ptr(), gt["root_trans"].data_ptr(), gt["kp3d"].data_ptr(), gt["mask"].data_ptr()
    d.loss, d.d_pred, d.errors, d.losses = loss.data_ptr(), grad.data_ptr(), errors.data_ptr(), losses.data_ptr()
    d.B, d.W, d.J, d.want_grad = pred.shape[0], pred.shape[1], gt["kp3d"].shape[1], 1
    kps = o["kps_need_depth"]
    if kps is not None:
        d.nk = len(kps)
        for i, k in enumerate(kps):
            d.kp_index[i] = k
    d.depth_loss, d.xy_loss = nv.DEPTH_LOSS_KINDS[o["depth_loss_func"]], nv.XY_LOSS_KINDS[o["xy_loss_func"]]
    d.root_col = 2 if o["xy_loss_func"] else (kps.index(3) if kps else 0)
    d.offset, d.capacity, d.batch_index, d.batch_capacity = offset, errors.shape[1], batch_index, losses.shape[0]
    nv.call("hrp_depth_loss", C.byref(d), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("mode", ["plain", "xy", "mkp"])
def test_bit_reproducible_across_runs_offsets_and_graph_replay(mode):
    B = 300
    o = dict(MODES[mode], depth_loss_func="mse" if mode == "mkp" else "l1")
    if mode == "xy":
        o["xy_loss_func"] = "mse"
    pred, gt = random_case(B, mode, 7)
    pred, gt = pred.to(DEV), {k: v.contiguous() for k, v in to_dev(gt).items()}

    def outputs():
        return (torch.zeros(1, device=DEV), torch.zeros_like(pred), torch.zeros(3, 700, device=DEV), torch.zeros(4, device=DEV))
    a, b, c = outputs(), outputs(), outputs()
    launch(pred, gt, o, a, 0, 0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch(pred, gt, o, b, 311, 3)               # another offset, another batch row
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(pred, gt, o, c, 400, 1)
    for t in c:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(a[0]).all() and a[0].item() > 0 and a[1].abs().sum().item() > 0
    for other, off, row in ((b, 311, 3), (c, 400, 1)):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
        assert torch.equal(a[2][:, :B], other[2][:, off:off + B]) and a[3][0].item() == other[3][row].item() == a[0].item()
        assert not other[2][:, :off].any() and not other[2][:, off + B:].any()


def test_farward_loss_end_to_end_on_a_real_rootnet():
    """The shipped options (l1, no xy branch, extended bbox, root 3) at B = 2, 256 x 256: finite gradients everywhere, and the
    loss of depth_l1_loss on the same output."""
    from synth import synth_state_dict
    from hrpe_amd.lib.core import depthnet as dn
    from hrpe_amd.lib.core.function import depth_l1_loss
    from hrpe_amd.lib.models.depth_net import get_rootnet
    m = get_rootnet("hrnet32")
    m.load_state_dict(synth_state_dict(m.state_dict()))
    m = m.to(DEV)
    outs = []
    m.register_forward_hook(lambda mod, inp, out: outs.append(out))
    batch = fx.batch_of("train", 0)
    for k, v in list(batch["root"].items()):
        batch["root"][k] = v[:2]
    for k in ("TCO", "K_original", "bbox_strict_bounded_original", "valid_mask"):
        batch[k] = batch[k][:2]
    batch["root"]["images"] = torch.randint(0, 256, (2, 3, 256, 256), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    args = fx.run_args("l1")
    loss = dn.farward_loss(args, batch, DEV, m, train=True)
    loss.backward()
    assert m.training and len(outs) == 1 and outs[0].shape == (2, 1) and torch.isfinite(loss)
    missing = [n for n, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    gt_depth = batch["root"]["keypoints_3d"][:, 3, 2:3].to(DEV)
    want = depth_l1_loss(outs[0].detach(), gt_depth)
    report("end to end loss", loss.item(), want.item())
    np.testing.assert_allclose(loss.item(), want.item(), rtol=fx.LOSS_RTOL, atol=0)


def test_validate_over_a_list_loader():
    from hrpe_amd.lib.core import depthnet as dn
    run = "xy_l1"
    args = fx.run_args(run)
    loader = [fx.batch_of("val", i) for i in (0, 2)]
    preds = [fx.pred_of(run, "val", i) for i in (0, 2)]
    host_writer = fx.Recorder()
    want = dn.validate(args, 2, "photo", loader, fx.StubModel(preds), host_writer, "cpu")
    model, writer = fx.StubModel([p.to(DEV) for p in preds]).to(DEV), fx.Recorder()
    model.train()
    got = dn.validate(args, 2, "photo", loader, model, writer, DEV)
    assert model.training and model.calls == 2 and all(k.is_cuda for k in model.k_values) and model.inputs[0].dtype == torch.uint8
    assert sorted(writer.scalars) == sorted(f"Val/{t}_photo" for t in fx.VAL_TAGS)
    np.testing.assert_allclose(writer.scalars["Val/rootz_loss_photo"][0], host_writer.scalars["Val/rootz_loss_photo"][0],
                               rtol=fx.LOSS_RTOL, atol=0)
    for tag in fx.VAL_TAGS[1:]:
        np.testing.assert_allclose(writer.scalars[f"Val/{tag}_photo"][0], host_writer.scalars[f"Val/{tag}_photo"][0], rtol=1e-6, atol=0)
    assert got == writer.scalars["Val/mean_depth_error_photo"][0]
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    out = dn.farward_loss(args, loader[0], DEV, model, train=False)            # without an evaluator: this batch's errors alone
    assert len(out) == 4 and all(t.is_cuda for t in out) and all(e.shape == (4,) for e in out[1:])
