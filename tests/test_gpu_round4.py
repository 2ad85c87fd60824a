"""Round-4 GPU parity tests.

* TWO iterations of the reference's trainers (scripts/train_depthnet.py:105, 231-250, 316-322 with depthnet.yaml - BASELINE.json
  configs[0]: B = 4, clip 1.0, Adam 1e-4 - and scripts/train_full.py:42, 56-66 with full.yaml, clip 5.0, B = 2) against the
  fixtures the reference itself wrote (tests/golden/gen_golden.py depthnet_2iter / full_2iter): forward -> loss -> backward ->
  clip -> Adam -> forward with repacked weights and updated running statistics, end to end, with hrpe_amd.optim.FusedClipAdam
  and with torch.optim.Adam + clip_grad_norm_.  fp32 tolerances: loss 1e-3 (relative), gradient norm 2e-2, parameter updates:
  median error < 5 % of the mean update; Adam's first steps are ~ lr * sign(g), so elements whose reference gradient (recorded in
  the fixture since round 5) is below 20 % of the tensor's mean |g| are left out, and at most 3 % of the remaining samples may
  miss by more than half a step (measured <= 2.3 %; gate 3 %).
* The benchmarked bf16 configuration: end-to-end key-point error in pixels, gated per key-point.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from synth import synth_inputs, synth_state_dict
import test_gpu_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


# measured (fp32, deterministic; the worst tensor is the DepthNet's stem convolution at B = 4): 4.3 % of ALL sampled elements miss;
# with the floor at 0.05 / 0.1 / 0.2 of the tensor's mean |g|: 2.2 / 1.9 / 1.1 % of the kept ones (90 / 82 / 68 % kept)
GRAD_FLOOR = float(os.environ.get("HRP_TEST_GRAD_FLOOR", "0.2"))


def two_iterations(model, loss_fn, clip, g, fused):
    from hrpe_amd.optim import FusedClipAdam
    params = [p for p in model.parameters() if p.requires_grad]
    named = dict(model.named_parameters())
    picks = [k.split(":")[1] for k in g.files if k.startswith("upd:") and k.endswith(":val")]
    p0 = {n: named[n].detach().clone() for n in picks}
    opt = FusedClipAdam(params, lr=1e-4, max_norm=clip) if fused else torch.optim.Adam(params, lr=1e-4)
    for it in range(2):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        if fused:
            opt.step()
            norm = float(opt.total_norm())
        else:
            norm = float(torch.nn.utils.clip_grad_norm_(params, clip))
            opt.step()
        np.testing.assert_allclose(loss.item(), g[f"loss{it + 1}"], rtol=1e-3, err_msg=f"loss of iteration {it + 1}")
        np.testing.assert_allclose(norm, g[f"grad_norm{it + 1}"], rtol=2e-2, err_msg=f"gradient norm of iteration {it + 1}")
    for n in picks:
        upd = (named[n].detach() - p0[n]).reshape(-1).cpu()[g[f"upd:{n}:idx"]].numpy()
        err = np.abs(upd - g[f"upd:{n}:val"])
        am = g[f"upd:{n}:absmean"]
        # Adam's first steps move an element by ~ lr * sign(g): an element whose REFERENCE gradient is at noise level (below
        # GRAD_FLOOR of the tensor's mean |g| in either iteration; the fp32 gradients of this 330-layer chain carry ~1e-2 of
        # relative rounding noise, test_gpu_model.py) has no well-defined sign and is left out; of the others at most 2 % may
        # miss by more than half a step (round 4 allowed 10 % of ALL elements).  The count is small and discrete:
        # the stem's conv1.weight - the end of the longest chain - keeps 174 elements, of which 2, 3 or 4 miss depending on the
        # summation order of the fp32 head launches (round 6: batched incre modules 1.1 % -> 2.3 % / 1.7 %): the gate is 3 %
        ok = np.ones(err.shape, bool)
        for it in (1, 2):
            ok &= np.abs(g[f"grad{it}:{n}:val"]) >= GRAD_FLOOR * g[f"grad{it}:{n}:absmean"]
        assert np.median(err) < 0.05 * am, (n, float(np.median(err)), float(am))
        if ok.sum() >= 32:
            miss = float(np.mean(err[ok] > 0.5 * am))
            print(f"  {n:60s} kept {int(ok.sum()):3d} / {len(ok)}  miss {miss:.3f}  (without the floor: {float(np.mean(err > 0.5 * am)):.3f})")
            assert miss <= 0.03, (n, miss, int(ok.sum()), float(am))
    sd = model.state_dict()
    for key in g.files:
        if key.startswith("buf:") and "num_batches" not in key:
            # (after two Adam steps of ~ lr * sign(g) per element: a few 1e-5 of absolute drift on statistics of O(0.1))
            np.testing.assert_allclose(sd[key[4:]].reshape(-1)[:64].cpu().numpy(), g[key], rtol=2e-3, atol=5e-5)
        if key.startswith("buf:") and "num_batches" in key:
            assert int(sd[key[4:]]) == int(g[key][0]) == 2


@pytest.mark.parametrize("fused", [True, False], ids=["FusedClipAdam", "torch.optim.Adam"])
def test_depthnet_two_iterations_golden(fused):
    from hrpe_amd.lib.models.depth_net import get_rootnet
    g = load("golden_depthnet_2iter.npz")
    m = get_rootnet("hrnet32")
    m.load_state_dict(synth_state_dict(m.state_dict()))
    m = m.to(DEV).train()
    x, _, kv, _ = synth_inputs(4)
    x, kv, gt = x.to(DEV), kv.to(DEV), torch.tensor(g["gt_depth"]).to(DEV)
    two_iterations(m, lambda: torch.nn.functional.l1_loss(m(x, kv) / 1000.0, gt), 1.0, g, fused)


@pytest.mark.parametrize("fused", [True, False], ids=["FusedClipAdam", "torch.optim.Adam"])
def test_full_two_iterations_golden(fused):
    from hrpe_amd.lib.core.function import compute_k_values, full_loss
    from hrpe_amd.lib.utils.geometries import rotmat_to_rot6d
    g = load("golden_full_2iter.npz")
    m = M.build_full().train()
    rng = np.random.Generator(np.random.PCG64(2024))
    x_reg = (torch.tensor(rng.integers(0, 256, (2, 3, 256, 256)).astype(np.float32)) / 255.).to(DEV)
    x_root = (torch.tensor(rng.integers(0, 256, (2, 3, 256, 256)).astype(np.float32)) / 255.).to(DEV)
    K = torch.tensor(g["in:K"]).to(DEV)
    kv = compute_k_values(K[:, 0, 0], K[:, 1, 1], torch.tensor(g["in:bbox"]).to(DEV))
    q, R, t = [torch.tensor(g[k]).to(DEV) for k in ("in:q", "in:R", "in:t")]
    kp3d, kp2d, mask = [torch.tensor(g[k]).to(DEV) for k in ("in:kp3d", "in:kp2d", "in:mask")]
    gt = dict(pose=q, root_rot=m.robot.get_rotation_at_specific_root(q, rotmat_to_rot6d(R), t, root=3),
              root_trans=kp3d[:, 3], root_uv=kp2d[:, 3], kp3d=kp3d, kp2d=kp2d, mask=mask)
    two_iterations(m, lambda: full_loss(m(x_reg, x_root, kv, K), gt, K)[0], 5.0, g, fused)


def _bf16_px_by_keypoint():
    """-> per key-point max |uv - uv_fp64| in pixels of the bf16 path on the reference's eval fixture (B = 2), computed exactly as
    bench.py's `max_px_err.bf16_by_keypoint` (the network's FK key-points against the reference's float64 run, both projected
    with K, lib/utils/transforms.py:17-21)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    r = bench.keypoint_px_error(torch.device(DEV), [("bf16", torch.bfloat16)])
    return r["bf16_by_keypoint"], r


def test_bf16_keypoint_0_documents_known_bf16_defect():
    """The benchmarked precision, in pixels.  This test DOCUMENTS A KNOWN DEFECT of the bf16 mode against the north star's pixel bar
    (VERDICT r4 weak #1, item 4c); it does not claim the bar is met: bench.py --full prints "px_bar_met": {"bf16": false, "fp32": true}.
    Six of the seven key-points of the fixture stay below 0.5 px (gated).  Key-point 0 sits 0.13 m in front of the camera (f = 800 px:
    1 mm of root depth is 3 px) and is off by 4.5 px in bf16 (gated at 5.5 so that it cannot get worse unnoticed).  What round 5
    measured about closing it: the DepthNet's head in fp32 0.92 px (+6.6 ms), the WHOLE DepthNet in fp32
    (HRP_DEPTHNET_FP32_FROM=1) still 2.4 px at 92 ms per step - the rest is the bf16 regression trunk's pose / rotation error seen
    from 0.13 m; a CPU emulation of the storage precisions (tools/emulate_bf16_modes.py) puts an fp32 residual stream at 0.9 px and
    bf16 WEIGHTS alone (every activation fp32) at 2.0 px.  No mode with bf16 operands meets 0.5 px on this key-point; the mode that
    does is fp32 (0.0011 px, tests/test_gpu_round3.py), whose step bench.py --full times as `fp32_step` (133 ms, 0.43 of the fp32 matrix peak)."""
    from hrpe_amd.lib.models.backbones import HRnet
    by_kp, r = _bf16_px_by_keypoint()
    print("\nbf16 px error by key-point:", by_kp)
    assert by_kp[0] < 5.5 and max(by_kp[1:]) < 0.5, by_kp
    saved = HRnet.HEAD_FP32
    try:
        HRnet.HEAD_FP32 = True
        by_kp2, _ = _bf16_px_by_keypoint()
    finally:
        HRnet.HEAD_FP32 = saved
    print("with the DepthNet head in fp32:", by_kp2)
    assert by_kp2[0] < 1.3 and max(by_kp2[1:]) < 0.5, by_kp2


def _train_curve(dtype, steps, B=8, nbatches=4, lr=1e-4):
    """`steps` training steps of the full network (synthetic batches of bench.py, the loss of lib/core/function.py:191-322, clip 5 +
    Adam 1e-4, no dropout) over `nbatches` DIFFERENT batches visited in turn -> losses.  Same seeded weights and batches for every call."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from hrpe_amd.lib.core.function import compute_k_values, full_loss
    from hrpe_amd.lib.utils.geometries import rotmat_to_rot6d
    from hrpe_amd.optim import FusedClipAdam
    m = M.build_full().set_compute_dtype(dtype).train()
    batches = []
    for b in range(nbatches):
        d = {k: torch.tensor(v).to(DEV) for k, v in bench.synthetic_batch(B, 4242 + 17 * b).items()}
        K = d["K"]
        kv = compute_k_values(K[:, 0, 0], K[:, 1, 1], d["bbox"])
        rot6 = rotmat_to_rot6d(d["R"])
        with torch.no_grad():
            kp3d, kp2d = m.robot.get_keypoints_and_projection(d["q"], rot6, d["t"], K, root=0)
            gt = dict(pose=d["q"], root_rot=m.robot.get_rotation_at_specific_root(d["q"], rot6, d["t"], root=3),
                      root_trans=kp3d[:, 3].clone(), root_uv=kp2d[:, 3].clone(), kp3d=kp3d, kp2d=kp2d, mask=torch.ones(B, 7, device=DEV))
        batches.append((d, kv, K, gt))
    opt = FusedClipAdam([p for p in m.parameters() if p.requires_grad], lr=lr, max_norm=5.0)
    losses = []
    for it in range(steps):
        d, kv, K, gt = batches[it % nbatches]
        opt.zero_grad()
        loss, _ = full_loss(m(d["x_reg"], d["x_root"], kv, K), gt, K)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return np.array(losses)


def test_bf16_training_follows_the_fp32_loss_curve():
    """80 optimizer steps in fp32 and in bf16 from the same weights over the same FOUR batches visited in turn, compared through the
    per-batch median loss of each window of five visits (20 steps).

    Learning rate 2e-5, not the trainers' 1e-4 (scripts/train_full.py:42): at 1e-4 this synthetic problem (random weights, B = 8,
    train-mode BatchNorm) is CHAOTIC - round 6 measured four runs of the SAME fp32 arithmetic that differ only in summation order
    (fused / unfused regressors, pooled / re-pooled fuse gradients: tools/curve_ab.py) ending between 0.77 and 0.95 of their first
    window, with first-window medians 10 % apart; the 10 % / 30 % bands of round 5 were inside that spread and the test could fail
    for either precision.  At 2e-5 the curves are smooth, two runs repeat bit for bit, and bf16 can be held to fp32 for real:
    measured window ratios (mean over the batches) 1.00, 0.97, 0.99, 0.99, worst single batch 0.86, falls 0.82 (fp32) / 0.81 (bf16).
    Gates: every window within 8 %, every batch of every window within 20 %, both falls below 0.9."""
    n, nb, vis = 80, 4, 5
    f32 = _train_curve(torch.float32, n, nbatches=nb, lr=2e-5)
    b16 = _train_curve(torch.bfloat16, n, nbatches=nb, lr=2e-5)
    nwin = n // (nb * vis)
    med = lambda v, k, w: float(np.median(v[k::nb][w * vis:(w + 1) * vis]))      # noqa: E731
    print("\nwindow   bf16 / fp32 median ratio per batch          mean")
    ratios, single = [], []
    for w in range(nwin):
        r = [med(b16, k, w) / med(f32, k, w) for k in range(nb)]
        single += r
        ratios.append(float(np.mean(r)))
        print(f"{w:4d}     " + " ".join(f"{x:8.3f}" for x in r) + f"   {ratios[-1]:8.3f}")
    for v, name in ((f32, "fp32"), (b16, "bf16")):
        fall = float(np.mean([med(v, k, nwin - 1) / med(v, k, 0) for k in range(nb)]))
        print(f"{name}: last / first window median, mean over the batches: {fall:.3f}")
        assert fall < 0.9, (name, fall)
    assert all(abs(r - 1.0) < 0.08 for r in ratios), ratios
    assert all(abs(r - 1.0) < 0.20 for r in single), single


def test_full_train_step_with_frozen_batchnorm_golden():
    """BASELINE config 5's way of training (scripts/train_sim2real.py:139-146): model.train() with every BatchNorm module in
    eval() - running statistics in the forward pass and gradients THROUGH them (dx = g * scale, dgamma = sum g * xhat with the
    running mean / variance, dbeta = sum g).  Fixture: the reference's own training step run that way
    (tests/golden/gen_golden.py full_train_bn_eval): forward 8-tuple, loss terms, sampled gradients, untouched running statistics.
    fp32 tolerances as test_full_train_step_golden (no batch statistics: no B = 2 amplification, but the same summaries)."""
    from hrpe_amd.lib.core.function import compute_k_values, full_loss
    from hrpe_amd.lib.utils.geometries import rotmat_to_rot6d
    g = load("golden_full_train_bn_eval.npz")
    m = M.build_full().train()
    n_bn = 0
    for mod in m.modules():          # the reference's own loop (scripts/train_sim2real.py:144-146): these ARE torch.nn.BatchNorm2d
        if isinstance(mod, torch.nn.BatchNorm2d) or isinstance(mod, torch.nn.BatchNorm1d):
            mod.eval()
            n_bn += 1
    assert n_bn > 600
    rng = np.random.Generator(np.random.PCG64(2024))
    x_reg = (torch.tensor(rng.integers(0, 256, (2, 3, 256, 256)).astype(np.float32)) / 255.).to(DEV)
    x_root = (torch.tensor(rng.integers(0, 256, (2, 3, 256, 256)).astype(np.float32)) / 255.).to(DEV)
    K = torch.tensor(g["in:K"]).to(DEV)
    kv = compute_k_values(K[:, 0, 0], K[:, 1, 1], torch.tensor(g["in:bbox"]).to(DEV))
    q, R, t = [torch.tensor(g[k]).to(DEV) for k in ("in:q", "in:R", "in:t")]
    kp3d, kp2d, mask = [torch.tensor(g[k]).to(DEV) for k in ("in:kp3d", "in:kp2d", "in:mask")]
    gt = dict(pose=q, root_rot=m.robot.get_rotation_at_specific_root(q, rotmat_to_rot6d(R), t, root=3),
              root_trans=kp3d[:, 3], root_uv=kp2d[:, 3], kp3d=kp3d, kp2d=kp2d, mask=mask)
    sd0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    pred = m(x_reg, x_root, kv, K)
    for n, p in zip(M.NAMES8, pred):
        ref = g["fwd:" + n]
        err = np.abs(p.detach().cpu().numpy() - ref).max() / (np.abs(ref).max() + 1e-12)
        assert err < 1e-3, f"forward {n}: rel err {err}"
    loss, terms = full_loss(pred, gt, K)
    for k, v in terms.items():
        np.testing.assert_allclose(v.item(), g["term:" + k], rtol=2e-3, err_msg=k)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-3)
    loss.backward()
    params = dict(m.named_parameters())
    checked = 0
    for key in g.files:
        if key.startswith("grad:") and key.endswith(":val"):
            name = key.split(":")[1]
            M.summary_check(params[name].grad, g, f"grad:{name}:", M.GRAD_TOL, what="frozen-BatchNorm ")
            checked += 1
    assert checked >= 10
    for k, v in m.state_dict().items():          # eval-mode BatchNorm: the running statistics do not move
        if "running" in k:
            assert torch.equal(v, sd0[k]), k


@pytest.mark.parametrize("case,func", [("iou_align", "mse_mean"), ("mse_mean", "mse_mean"), ("bce", "bce"), ("mse_sum", "mse_sum")])
def test_sim2real_mask_loss_kernel_golden(case, func):
    """hrp_sim2real_loss (mask / IoU / scale / 3-D alignment losses of the self-supervised trainer and their analytic gradient,
    scripts/train_sim2real.py:435-468) against the fixture written by executing those statements of the reference on seeded
    silhouettes (two of the six images trip the scale filter).  fp32 sums over 768 pixels in another order: 2e-5 on the terms,
    gradients 1e-4 of their scale; a second call gives bit-identical results (fixed summation order)."""
    from hrpe_amd.lib.core.function import sim2real_mask_loss
    g = load("golden_sim2real_loss.npz")
    r = torch.tensor(g["in:rendered"]).to(DEV).requires_grad_(True)
    a, b = torch.tensor(g["in:kp3d"]).to(DEV).requires_grad_(True), torch.tensor(g["in:kp3d_int"]).to(DEV).requires_grad_(True)
    seg = torch.tensor(g["in:seg"]).unsqueeze(1).to(DEV)
    wm, wi, ws, wa = [float(v) for v in g[f"{case}:weights"]]
    w = dict(mask=wm, iou=wi, scale=ws, align=wa)
    loss, terms = sim2real_mask_loss(r, seg, a, b, func, w)
    for k, v in terms.items():
        np.testing.assert_allclose(v.item(), g[f"{case}:{k}"], rtol=2e-5, err_msg=k)
    np.testing.assert_allclose(loss.item(), g[f"{case}:loss"], rtol=2e-5)
    (loss * 1.0).backward()
    for t, key in ((r, "d_rendered"), (a, "d_kp3d"), (b, "d_kp3d_int")):
        ref = g[f"{case}:{key}"]
        err = np.abs(t.grad.cpu().numpy() - ref).max()
        assert err <= 1e-4 * np.abs(ref).max() + 1e-12, (key, err, np.abs(ref).max())
    loss2, terms2 = sim2real_mask_loss(r.detach().requires_grad_(True), seg, a.detach(), b.detach(), func, w)
    assert torch.equal(loss2, loss.detach()) and all(torch.equal(terms2[k], terms[k]) for k in terms)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(64, 64, 2, 30, 40, 2, True), (128, 96, 4, 30, 40, 1, False), (32, 32, 2, 13, 9, 3, False),
                                  (64, 32, 4, 60, 80, 1, False), (256, 256, 2, 60, 80, 1, False)],
                         ids=lambda c: "c%d-%d_d%d_%dx%d" % c[:5])
def test_dilated_conv(case, dtype):
    """Atrous 3x3 convolutions (dilation 2 / 4: layer3 / layer4 of DeepLabv3's ResNet-50 with output stride 8, dilation 12: the
    first ASPP branch; reference lib/models/ctrnet/keypoint_seg_resnet.py:103-149 builds torchvision's deeplabv3_resnet50, which
    the self-supervised trainer runs frozen and detached, scripts/train_sim2real.py:412; ASPP's dilations 12 / 24 / 36 exceed
    every tile's halo and are refused loudly - test below) on the general tile program, against
    torch fp32 on the CPU: the forward pass for every case (what the frozen mask network needs), data and weight gradient where
    flagged (the weight-gradient kernel's tiles take halos up to dilation 2 at these sizes and say so otherwise)."""
    import torch.nn.functional as F
    from hrpe_amd.lib.models.backbones.HRnet import Conv2d
    cin, cout, dil, H, W, N, backward = case
    g = torch.Generator().manual_seed(cin * 1000 + dil)
    conv = Conv2d(cin, cout, 3, bias=False, dilation=dil)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(cin * 9))
    x = torch.randn(N, cin, H, W, generator=g)
    wr, xr = conv.weight.detach().clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, padding=dil, dilation=dil)
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    conv = conv.to(DEV).set_compute_dtype(dtype)
    tol = 2e-4 if dtype == torch.float32 else 4e-2

    def rel(a, b):
        return ((a.detach().float().cpu() - b.detach()).abs().max() / (b.detach().abs().max() + 1e-12)).item()
    with torch.no_grad():
        y = conv.eval()(x.to(DEV))
    assert y.shape == yr.shape and rel(y, yr) < tol, rel(y, yr)
    if backward:
        xd = x.to(DEV).requires_grad_(True)
        y = conv.train()(xd)
        assert rel(y, yr) < tol
        (y * gy.to(DEV)).sum().backward()
        assert rel(xd.grad, xr.grad) < tol, ("data gradient", rel(xd.grad, xr.grad))
        assert rel(conv.weight.grad, wr.grad) < tol, ("weight gradient", rel(conv.weight.grad, wr.grad))


def test_mesh_pose_kernel_golden():
    """hrp_mesh_pose (URDFRobot.pose_mesh: the posed robot mesh in the camera frame for a whole batch in one launch) against the
    reference-generated fixture (link poses of the reference's kinematics, camera pose recorded from the reference's
    get_rendered_mask_single_image_at_specific_root, roots 0 and 3, two samples behind the camera) and against pinhole
    projection of its own output.  fp32: 5e-6 m."""
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    g = load("golden_mesh_pose.npz")
    robot = URDFRobot("panda")
    q, r6, t = [torch.tensor(g[k]).to(DEV) for k in ("q", "rot6d", "t")]
    verts, vl = torch.tensor(g["verts"]).to(DEV), torch.tensor(g["vert_link"]).to(DEV)
    K = torch.tensor([[160.0, 0, 160.0], [0, 160.0, 120.0], [0, 0, 1.0]]).repeat(q.shape[0], 1, 1).to(DEV)
    for root in (0, 3):
        xyz, uv = robot.pose_mesh(q, r6, t, verts, vl, root=root, K=K)
        np.testing.assert_allclose(xyz.cpu().numpy(), g[f"cam_root{root}"], atol=5e-6, err_msg=f"root {root}")
        ref_uv = torch.stack([160.0 * xyz[..., 0] / xyz[..., 2] + 160.0, 160.0 * xyz[..., 1] / xyz[..., 2] + 120.0], -1)
        np.testing.assert_allclose(uv.cpu().numpy(), ref_uv.cpu().numpy(), rtol=1e-5, atol=1e-3)
        assert (xyz[[3, 7], :, 2] > 0).all()                   # mirrored in front of the camera
    big = torch.randn(5000, 3, device=DEV) * 0.05              # more vertices than one workgroup pass
    bl = torch.randint(0, 9, (5000,), device=DEV, dtype=torch.uint8)
    a = robot.pose_mesh(q, r6, t, big, bl, root=3)
    b = robot.pose_mesh(q, r6, t, big[:100], bl[:100], root=3)
    assert torch.equal(a[:, :100], b)


@pytest.mark.parametrize("tag", ["near", "far"])
def test_fused_pose_loss_on_prescribed_predictions_golden(tag):
    """hrp_pose_loss (ten terms + analytic gradient, one launch) directly against the reference's step function run on a stand-in
    model with prescribed outputs (golden_pose_loss.npz): `far` is the damped branch of function.py:245-251, which the network
    fixtures never reach.  fp32: terms 2e-5, gradients 2e-4 (+ 1e-5 of the tensor's largest entry)."""
    from hrpe_amd.lib.core.function import full_loss
    from hrpe_amd.lib.utils.geometries import rotmat_to_rot6d
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    g = load("golden_pose_loss.npz")
    robot = URDFRobot("panda")
    K = torch.tensor(g["in:K"]).to(DEV)
    q, R, t = [torch.tensor(g[k]).to(DEV) for k in ("in:q", "in:R", "in:t")]
    kp3d, kp2d, mask = [torch.tensor(g[k]).to(DEV) for k in ("in:kp3d", "in:kp2d", "in:mask")]
    gt = dict(pose=q, root_rot=robot.get_rotation_at_specific_root(q, rotmat_to_rot6d(R), t, root=3),
              root_trans=kp3d[:, 3], root_uv=kp2d[:, 3], kp3d=kp3d, kp2d=kp2d, mask=mask)
    pred = [torch.tensor(g[f"{tag}:pred:{n}"]).to(DEV).requires_grad_(True) for n in M.NAMES8]
    loss, terms = full_loss(pred, gt, K)
    for k, v in terms.items():
        np.testing.assert_allclose(float(v), g[f"{tag}:term:{k}"], rtol=2e-5, err_msg=k)
    np.testing.assert_allclose(loss.item(), g[f"{tag}:loss"], rtol=2e-5)
    loss.backward()
    for n, p in zip(M.NAMES8, pred):
        ref = g[f"{tag}:grad:{n}"]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-7 + 1e-5 * np.abs(ref).max(), err_msg=n)


def test_fk_kernel_with_quaternion_rotation_golden():
    """hrp_fk_project_rot_fwd / _bwd with rot_dim = 4 (the rotation_dim == 4 variant, reference urdf_robot.py:86-92, 118-138) against
    the reference fixture: key-points 3e-6 m, gradients, the re-rooted rotation as a quaternion."""
    from hrpe_amd.lib.utils.transforms import point_projection_from_3d_tensor
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    g = load("golden_fk_quat.npz")
    robot = URDFRobot("panda")
    q, r, t, K = [torch.tensor(g[k]).to(DEV) for k in ("q", "rot6d", "t", "K")]
    assert r.shape[1] == 4
    for root in (0, 3):
        tq, tr, tt = [x.clone().requires_grad_(True) for x in (q, r, t)]
        xyz = robot.get_keypoints_root(tq, tr, tt, root=root)
        uv = point_projection_from_3d_tensor(K, xyz)
        np.testing.assert_allclose(xyz.detach().cpu().numpy(), g[f"xyz_root{root}"], atol=3e-6)
        ((xyz * torch.tensor(g["w_xyz"]).to(DEV)).sum() + (uv * torch.tensor(g["w_uv"]).to(DEV)).sum()).backward()
        for name, x in (("gq", tq), ("grot", tr), ("gt", tt)):
            ref = g[f"{name}_root{root}"]
            np.testing.assert_allclose(x.grad.cpu().numpy(), ref, atol=3e-4 * max(1.0, np.abs(ref).max()), rtol=2e-3)
        rr = robot.get_rotation_at_specific_root(q, r, t, root=root).cpu().numpy()
        ref = g[f"rootrot_root{root}"]
        # geometries.py:63-82 divides the antisymmetric part by 4 w with w = sqrt(1 + trace) / 2: matrix entries that differ by
        # one fp32 ulp (1e-7) move the quaternion by ~1e-7 / w - the fixture holds samples with w = 0.02
        tol = 3e-6 + 1e-6 / np.maximum(np.abs(ref[:, :1]), 1e-3)
        assert (np.abs(rr - ref) <= tol).all(), float((np.abs(rr - ref) / tol).max())


def test_full_network_with_quaternion_rotation_golden():
    """rotation_dim = 4 (reference full_net.py:129-131, 186-189; function.py:63-64): inference 8-tuple against
    golden_full_eval_quat.npz (3e-4) and one training step against golden_full_train_quat.npz (loss terms 2e-3 - loss_rot is the
    mean squared quaternion difference -, sampled gradients as the 6-D fixture)."""
    from hrpe_amd.lib.core.function import compute_k_values, full_loss
    from hrpe_amd.lib.utils.geometries import rotmat_to_quat
    from synth import synth_inputs
    g = load("golden_full_eval_quat.npz")
    m = M.build_full(rotation_dim=4).eval()
    x_reg, x_root, kv, K = synth_inputs(2)
    with torch.no_grad():
        out = m(x_reg.to(DEV), x_root.to(DEV), kv.to(DEV), K.to(DEV))
    assert out[1].shape[1] == 4
    for n, t in zip(M.NAMES8, out):
        ref = g[n]
        err = np.abs(t.cpu().numpy() - ref).max() / (np.abs(ref).max() + 1e-12)
        assert err < 3e-4, f"{n}: rel err {err}"
    g = load("golden_full_train_quat.npz")
    m = M.build_full(rotation_dim=4).train()
    rng = np.random.Generator(np.random.PCG64(2024))
    x_reg = (torch.tensor(rng.integers(0, 256, (2, 3, 256, 256)).astype(np.float32)) / 255.).to(DEV)
    x_root = (torch.tensor(rng.integers(0, 256, (2, 3, 256, 256)).astype(np.float32)) / 255.).to(DEV)
    K = torch.tensor(g["in:K"]).to(DEV)
    kv = compute_k_values(K[:, 0, 0], K[:, 1, 1], torch.tensor(g["in:bbox"]).to(DEV))
    q, R, t = [torch.tensor(g[k]).to(DEV) for k in ("in:q", "in:R", "in:t")]
    kp3d, kp2d, mask = [torch.tensor(g[k]).to(DEV) for k in ("in:kp3d", "in:kp2d", "in:mask")]
    gt = dict(pose=q, root_rot=m.robot.get_rotation_at_specific_root(q, rotmat_to_quat(R), t, root=3),
              root_trans=kp3d[:, 3], root_uv=kp2d[:, 3], kp3d=kp3d, kp2d=kp2d, mask=mask)
    pred = m(x_reg, x_root, kv, K)
    loss, terms = full_loss(pred, gt, K)
    for k, v in terms.items():
        np.testing.assert_allclose(v.item(), g["term:" + k], rtol=2e-3, err_msg=k)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-3)
    loss.backward()
    params = dict(m.named_parameters())
    for key in g.files:
        if key.startswith("grad:") and key.endswith(":val"):
            name = key.split(":")[1]
            M.summary_check(params[name].grad, g, f"grad:{name}:", M.GRAD_TOL, what="quaternion ")


def test_fp32_inference_is_bit_reproducible():
    """Two fresh fp32 models, the same inputs: identical 8-tuples, bit for bit.  (Until round 4 the 256-channel fuse layers at 8 x 8
    ran the conv path's split-K with FOUR atomically added fp32 partials - the order of the additions moved key-point 0 by up to
    1.5e-3 px from run to run and made test_fp32_keypoints_within_the_reference_fp32_noise_floor fail one run in six; the split
    is capped at two slices now, whose sum does not depend on the order.)"""
    from synth import synth_inputs
    x_reg, x_root, kv, K = [t.to(DEV) for t in synth_inputs(2)]
    outs = []
    for _ in range(3):
        m = M.build_full().eval()
        with torch.no_grad():
            outs.append([t.clone() for t in m(x_reg, x_root, kv, K)])
    for o in outs[1:]:
        for n, a, b in zip(M.NAMES8, o, outs[0]):
            assert torch.equal(a, b), n


def test_fp32_training_step_is_bit_reproducible():
    """Two fresh fp32 DepthNets, the same batch: identical loss and identical gradients for all 981 parameters.  (bf16 steps have
    been bit-reproducible since round 3; in fp32 the split-K of the skinny layers added its partials atomically ONTO gradients
    that accumulate - (y + a) + b against (y + b) + a - which made 897 of the 981 gradients differ in the last bits from run to run;
    such launches no longer split.)"""
    from hrpe_amd.lib.models.depth_net import get_rootnet
    x, _, kv, _ = synth_inputs(4)
    runs = []
    for _ in range(2):
        m = get_rootnet("hrnet32")
        m.load_state_dict(synth_state_dict(m.state_dict()))
        m = m.to(DEV).train()
        loss = torch.nn.functional.l1_loss(m(x.to(DEV), kv.to(DEV)) / 1000.0, torch.ones(4, 1, device=DEV))
        loss.backward()
        runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    bad = [n for n in runs[0][1] if not torch.equal(runs[0][1][n], runs[1][1][n])]
    assert len(runs[0][1]) > 900 and not bad, bad[:8]
