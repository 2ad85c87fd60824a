"""GPU tests of CtRNet's key-point branch (csrc/kp_readout.hip, PlanBuilder.kp_readout, KeyPointSegNet / seg_mask_inference.detect /
CtRNet.inference_*; reference lib/models/ctrnet/keypoint_seg_resnet.py:29-33, 75-100, 137-143, CtRNet.py:49-129).

The kernel is held to the float64 oracle of tests/kp_readout_oracle.py on EXACT operands (integers in -2 .. 2, weights times 2^-s: the
logits of a correct kernel are exact in bf16 MFMA and in fp32 in any order, so the maximum logit is compared with ==) and to the
reference's own output recorded in tests/golden/golden_kp_readout.npz:
  key-points within 4e-6 * scale of the oracle (the 2e-6 of test_softargmax_golden_and_backward on a coordinate range twice as wide;
  the reference itself stays 40 x inside), within 5e-6 * scale of the fixture; ms[..., 0] == the oracle's maximum;
  1 / ms[..., 1] within 2e-6 of the oracle's peak probability; two runs torch.equal.
The whole network is PARITY UNPINNED like the mask: its oracle is oracle/segnet.py, this repository's restatement."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kp_readout_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_kp_readout.npz"))
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def run_kernel(x, w, b, dtype, lim=O.LIM, size=O.SIZE, want_ms=True, x3=False):
    """x [B, Cin, Hin, Win], w [Cin, k, 4, 4], b [k] (host) -> kp [B, k, 2], ms [B, k, 2] (host).  The feature has a pitch of
    Cin + 8 whose padding holds 3.0 (never read by a correct kernel)."""
    from hrpe_amd import _native as nv
    B, cin, hin, win = x.shape
    k = w.shape[1]
    xt, pitch = O.nhwc(x, dtype)
    xt[..., cin:] = 3.0
    xd, wd, bd = xt.to(DEV), w.float().contiguous().to(DEV), b.float().to(DEV)
    dt = nv.HRP_BF16 if dtype == torch.bfloat16 else (nv.HRP_F32X3 if x3 else nv.HRP_F32)
    packed = torch.zeros(16 * cin * 32, dtype=dtype, device=DEV)
    nv.call("hrp_kp_readout_pack", wd.data_ptr(), cin, k, packed.data_ptr(), dt, None)
    wsb = int(nv.lib().hrp_kp_readout_ws(B, hin))
    ws = torch.full((wsb // 4 + 8,), float("nan"), device=DEV)          # (every partial the combine reads must have been written)
    kp = torch.full((B, k, 2), float("nan"), device=DEV)
    ms = torch.full((B, k, 2), float("nan"), device=DEV)
    nv.call("hrp_kp_readout_fwd", xd.data_ptr(), dt, B, hin, win, cin, pitch, packed.data_ptr(), bd.data_ptr(), k, float(lim[0]),
            float(lim[2]), float(size[0] // 2), float(size[1] // 2), kp.data_ptr(), ms.data_ptr() if want_ms else None, ws.data_ptr(),
            wsb, None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[wsb // 4:]).all()), "the kernel wrote behind its workspace"
    return kp.cpu(), ms.cpu()


def all_cases():
    from hrpe_amd import _native as nv
    return O.all_cases(nv.KP_STRIP_ROWS)


SCALE = torch.tensor([O.SIZE[0] // 2, O.SIZE[1] // 2], dtype=torch.float64)


def check_gates(kp, ms, want, where):
    err = ((kp.double() - want["kp"]).abs() / SCALE).max().item()
    perr = (1.0 / ms[..., 1].double() - want["pmax"]).abs().max().item()
    print(f"\n{where}: key-point error {err:.2e} (normalised), peak-probability error {perr:.2e}")
    assert err <= 4e-6, (where, err)
    assert torch.equal(ms[..., 0].double(), want["max"]), where
    assert perr <= 2e-6, (where, perr)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_operands_against_the_oracle_and_the_reference(dtype):
    """Every shape of the list (one K step with every tap at an edge, Cin not a power of two, odd sides, maximum k, the product's
    Cin, maps of 40, 70 and 131 columns - the second position tile, two and three passes over a workgroup's positions with the
    running sums rescaled in between -, the two strip-seam heights, the spikes at the last and the first output position of a
    narrow and of a 70-column map) in one element type."""
    from hrpe_amd import _native as nv
    for shape, spikes in all_cases():
        x, w, b, _ = O.operands(shape, spikes)
        want = O.readout64(x, w, b)
        kp, ms = run_kernel(x, w, b, dtype)
        where = f"{O.key(shape, spikes)} {dtype}"
        check_gates(kp, ms, want, where)
        gk = O.key(shape, spikes) + "_kp"
        if gk in GOLD.files:
            ferr = ((kp.double() - torch.from_numpy(GOLD[gk]).double()).abs() / SCALE).max().item()
            assert ferr <= 5e-6, (where, ferr)
        else:
            assert int(GOLD["strip"]) != nv.KP_STRIP_ROWS, gk      # only a seam shape of another strip height may be missing
        kp2, ms2 = run_kernel(x, w, b, dtype)
        assert torch.equal(kp, kp2) and torch.equal(ms, ms2), where
        if spikes:                                                # the two spiked channels sit on their corners
            k = shape[2]
            last = torch.tensor([(1.0 - O.LIM[0]) * SCALE[0], (1.0 - O.LIM[2]) * SCALE[1]])
            first = torch.tensor([(-1.0 - O.LIM[0]) * SCALE[0], (-1.0 - O.LIM[2]) * SCALE[1]])
            assert (kp[:, 0].double() - last).abs().max() < 1e-3 and (kp[:, k - 1].double() - first).abs().max() < 1e-3
            assert float((1.0 / ms[:, [0, k - 1], 1]).min()) > 1 - 1e-6


def test_fp32x3_plans_take_the_fp32_form_and_ms_may_be_null():
    shape = O.SHAPES[2]
    x, w, b, _ = O.operands(shape)
    kp, ms = run_kernel(x, w, b, torch.float32)
    kp3, ms3 = run_kernel(x, w, b, torch.float32, x3=True)
    assert torch.equal(kp, kp3) and torch.equal(ms, ms3)
    kpn, msn = run_kernel(x, w, b, torch.float32, want_ms=False)
    assert torch.equal(kp, kpn) and bool(torch.isnan(msn).all())
    kpd, _ = run_kernel(x, w, b, torch.float32, lim=(-1.0, 1.0, -1.0, 1.0), size=(97, 65))     # the module's default lim, odd sizes
    want = O.readout64(x, w, b, lim=(-1.0, 1.0, -1.0, 1.0), size=(97, 65))
    assert ((kpd.double() - want["kp"]).abs() / torch.tensor([48.0, 32.0], dtype=torch.float64)).max() <= 4e-6


def test_refusals_raise():
    from hrpe_amd import _native as nv
    t = torch.zeros(1 << 16, device=DEV)
    p = t.data_ptr()

    def fwd(**over):
        a = dict(x=p, dtype=nv.HRP_F32, B=1, Hin=2, Win=2, Cin=64, pitch=64, packed=p, bias=p, k=7, lim0=-1.0, lim2=-1.0, sx=8.0, sy=8.0,
                 kp=p, ms=None, ws=p, ws_bytes=1 << 16, stream=None)
        a.update(over)
        nv.call("hrp_kp_readout_fwd", *a.values())
    fwd()
    for over in (dict(Cin=48, pitch=48), dict(k=0), dict(k=33), dict(Hin=0), dict(Win=0), dict(B=0), dict(x=None), dict(packed=None),
                 dict(bias=None), dict(kp=None), dict(ws=None)):
        with pytest.raises(nv.HrpError, match="kp_readout_fwd"):
            fwd(**over)
    for over in (dict(Cin=48), dict(k=33), dict(w=None), dict(out=None)):
        a = dict(w=p, Cin=64, k=7, out=p, dtype=nv.HRP_F32, stream=None)
        a.update(over)
        with pytest.raises(nv.HrpError, match="kp_readout_pack"):
            nv.call("hrp_kp_readout_pack", *a.values())
    torch.cuda.synchronize()


def scaled_for_logit_range(heat_of, w):
    """The power of two that puts every channel's logit range (max - min over the positions) inside 5 .. 30"""
    heat = heat_of(w)
    rng = (heat.amax(dim=(2, 3)) - heat.amin(dim=(2, 3)))
    p = 2.0 ** round(float(torch.log2(12.0 / rng.median())))
    rng = rng * p
    assert 5.0 <= float(rng.min()) and float(rng.max()) <= 30.0, (float(rng.min()), float(rng.max()))
    return p


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_realistic_operands_within_the_derived_bound(dtype):
    """Normal features and weights rounded to the element type for both sides, Cin 2048, logit range per channel in 5 .. 30.  The
    accumulation error of a logit is at most eps = 4 Cin 2^-23 max sum |x w| (4 Cin products, fp32 accumulation); under a logit
    perturbation of at most eps every probability moves by a factor in [e^-2eps, e^2eps] and |coordinate| <= 1, so the key-point
    moves by at most (e^2eps - 1) * scale, plus the 4e-6 * scale of the softmax arithmetic itself.
    At K = 8192 the worst-case eps is 0.165 and the key-point bound 0.39 of the coordinate range: it is STRUCTURAL (a wrong tap, a
    lost K slice or a rounded logit moves a key-point by more), not a statement of accuracy.  What constrains the arithmetic in this
    test is the maximum logit, held to eps against float64; the accuracy of the soft-argmax is held on the exact operands above."""
    B, cin, k, hin, win = 2, 2048, 7, 6, 8
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, cin, hin, win, generator=g).to(dtype).double()
    w = torch.randn(cin, k, 4, 4, generator=g).double()
    b = torch.randn(k, generator=g).float().double()
    w = w * scaled_for_logit_range(lambda ww: F.conv_transpose2d(x, ww, b, stride=2, padding=1), w)
    w = w.to(dtype).double()                # (a power of two commutes with the rounding; the range check above holds to 2^-8)
    want = O.readout64(x, w, b)
    eps = 4 * cin * 2.0 ** -23 * float(F.conv_transpose2d(x.abs(), w.abs(), None, stride=2, padding=1).max())
    bound = (np.exp(2 * eps) - 1.0) + 4e-6
    kp, ms = run_kernel(x, w, b, dtype)
    err = ((kp.double() - want["kp"]).abs() / SCALE).max().item()
    print(f"\nrealistic {dtype}: eps {eps:.3e}, bound {bound:.3e}, error {err:.3e} (normalised); "
          f"max-logit error {(ms[..., 0].double() - want['max']).abs().max().item():.2e}")
    assert err <= bound, (err, bound)
    assert (ms[..., 0].double() - want["max"]).abs().max().item() <= eps


def make_conv_readout(cin0, cin, k, size):
    from hrpe_amd.lib.models.backbones.HRnet import Conv2d
    from hrpe_amd.lib.models.ctrnet.keypoint_seg_resnet import KeypointUpSample
    from hrpe_amd.runtime import PlannedModule

    class ConvReadout(PlannedModule):
        def __init__(self):
            super().__init__()
            self.conv = Conv2d(cin0, cin, 1, bias=False)
            self.read_out = KeypointUpSample(cin, k)

        def _build(self, pb, x):
            N, Cc, H, W = x.shape
            t = pb.image_input("x", N, Cc, H, W)
            feat = self.conv.emit(pb, t)
            kp, ms = self.read_out.emit(pb, feat, O.LIM, size)
            return ["x"], [("vec", kp, (N, k, 2)), ("vec", ms, (N, k, 2))], {"x": t}

        def forward(self, x):
            return self._run(x)
    return ConvReadout()


def exact_state(seed, cin0, cin, k, s):
    """A 1 x 1 convolution whose rows hold one +-1 each (its output stays integers in -2 .. 2) and exact read-out weights"""
    g = torch.Generator().manual_seed(seed)
    cw = torch.zeros(cin, cin0, 1, 1)
    src = torch.randint(0, cin0, (cin,), generator=g)
    cw[torch.arange(cin), src, 0, 0] = torch.randint(0, 2, (cin,), generator=g).float() * 2 - 1
    w = torch.randint(-2, 3, (cin, k, 4, 4), generator=g).float() * 2.0 ** -s
    b = torch.randint(-8, 9, (k,), generator=g).float() * 0.25
    return {"conv.weight": cw, "read_out.kps_score_lowres.weight": w, "read_out.kps_score_lowres.bias": b}


@pytest.mark.parametrize("dtype", DTYPES + ["fp32x3"], ids=IDS + ["fp32x3"])
def test_plan_integration_repacks_after_load_state_dict(dtype):
    """conv -> kp_readout in one plan on exact operands; a load_state_dict AFTER the first run must reach the packed read-out weight
    (Plan.run_prep) - also once the plan replays from its captured graph; gradients are refused."""
    cin0, cin, k, hin, win, s = 64, 96, 5, 5, 6, 4
    m = make_conv_readout(cin0, cin, k, O.SIZE).to(DEV).set_compute_dtype(dtype).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-2, 3, (2, cin0, hin, win), generator=g).float()
    for it, seed in enumerate((21, 22, 22, 22, 23)):            # (the fourth call replays the graph; the fifth repacks under it)
        sd = exact_state(seed, cin0, cin, k, s)
        m.load_state_dict(sd)
        kp, ms = m(x.to(DEV))
        feat = F.conv2d(x.double(), sd["conv.weight"].double())
        want = O.readout64(feat, sd["read_out.kps_score_lowres.weight"], sd["read_out.kps_score_lowres.bias"])
        check_gates(kp.cpu(), ms.cpu(), want, f"plan call {it} {dtype}")
    for p in m.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m(x.to(DEV))


# ---- the whole network ---------------------------------------------------------------------------------------------------------
NET_HW = (64, 96)
# measured on an MI355X: largest key-point error against the float64 read-out of oracle/segnet.py's features, in pixels
# of the 96 x 64 image; the gate is 4 x that
NET_MEASURED = {torch.float32: 7.2e-5, torch.bfloat16: 0.19}


def net_args():
    a = argparse.ArgumentParser().parse_args("")
    a.use_gpu, a.n_kp, a.height, a.width = True, 7, NET_HW[0], NET_HW[1]
    return a


def oracle_features(sd, x):
    """layer4 features of oracle/segnet.py's dilated ResNet-50 (the first lines of its deeplab_forward)"""
    from oracle import segnet as og
    b = "backbone.0."
    h = F.relu(og._bn(sd, b + "bn1", F.conv2d(x, sd[b + "conv1.weight"], stride=2, padding=3)))
    h = F.max_pool2d(h, 3, 2, 1)
    for name, blocks in og.layer_plan():
        for i, (stride, dil) in enumerate(blocks):
            h = og._bottleneck(sd, f"{b}{name}.{i}", h, stride, dil)
    return h


@pytest.fixture(scope="module")
def net_case():
    """Random initialisation (seeded), the read-out weight rescaled by a power of two so that every channel's logit range lies in
    5 .. 30, the oracle's features, key-points and segmentation: computed once, read by both element types."""
    from oracle import segnet as og
    from hrpe_amd.lib.models.ctrnet.keypoint_seg_resnet import KeyPointSegNet
    torch.manual_seed(1234)
    net = KeyPointSegNet(net_args()).eval()
    g = torch.Generator().manual_seed(6)
    img = torch.randn(2, 3, *NET_HW, generator=g) * 0.2       # (white noise alone leaves every peak in one corner of the map)
    img[0, :, 8:24, 60:84] += 3.0
    img[1, :, 40:56, 8:30] -= 3.0
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        feat = oracle_features(sd, img).double()
        wk, bk = "read_out.kps_score_lowres.weight", "read_out.kps_score_lowres.bias"
        sd[wk] = sd[wk] * scaled_for_logit_range(lambda ww: F.conv_transpose2d(feat, ww.double(), sd[bk].double(), stride=2, padding=1), sd[wk])
        want = O.readout64(feat, sd[wk], sd[bk], lim=net.lim, size=(NET_HW[1], NET_HW[0]))
        seg = og.deeplab_forward(sd, img)
    span = want["kp"].reshape(-1, 2).amax(0) - want["kp"].reshape(-1, 2).amin(0)
    assert float(span[0]) >= NET_HW[1] / 4 and float(span[1]) >= NET_HW[0] / 4, span      # the key-points use the image
    net.load_state_dict(sd)
    return net, img, want, seg


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_whole_network_keypoints_and_unchanged_segmentation(net_case, dtype):
    net, img, want, seg_ref = net_case
    m = net.to(DEV).set_compute_dtype(dtype)
    x = img.to(DEV)
    with torch.no_grad():
        none, seg_off = m(x)
        m.with_keypoints = True
        kp, seg_on = m(x)
        kp2, seg_call = m(x, keypoints=True)
        m.with_keypoints = False
        none2, seg_off2 = m(x)
    assert none is None and none2 is None and kp.shape == (2, 7, 2) and kp.dtype == torch.float32
    assert torch.equal(seg_on, seg_off) and torch.equal(seg_call, seg_off) and torch.equal(seg_off2, seg_off)
    assert torch.equal(kp, kp2)
    err = (kp.cpu().double() - want["kp"]).abs().max().item()
    serr = (seg_off.cpu() - seg_ref).abs().max().item()
    print(f"\nwhole network {dtype}: key-point error {err:.3e} px of {NET_HW[1]} x {NET_HW[0]}, segmentation logit error {serr:.2e}")
    assert err <= 4 * NET_MEASURED[dtype], err


def test_ctrnet_methods_and_detect():
    """CtRNet.inference_batch_images_seg_kp / inference_batch_images / inference_single_image, cTr_to_pose_matrix, to_valid_R_batch,
    and seg_mask_inference.detect against .forward (one plan, the same mask bit for bit)."""
    from hrpe_amd import _native as nv
    from hrpe_amd.lib.models.ctrnet.mask_inference import seg_mask_inference
    from hrpe_amd.lib.utils.BPnP import batch_project
    torch.manual_seed(5)
    m = seg_mask_inference((60.0, 60.0, 48.0, 32.0), "azure", image_hw=(128, 192), allow_random_init=True).to(DEV)
    img = torch.randint(0, 256, (2, 3, 128, 192), dtype=torch.uint8, device=DEV)
    prob = m(img)
    kp, prob_d, ms = m.detect(img)
    assert torch.equal(prob, prob_d) and torch.equal(m(img), prob)
    assert kp.shape == (2, 7, 2) and ms.shape == (2, 7, 2) and prob.shape == (2, 1, 64, 96)
    assert bool(((kp[..., 0] >= 0) & (kp[..., 0] <= 96) & (kp[..., 1] >= 0) & (kp[..., 1] <= 64)).all())
    assert bool((ms[..., 1] >= 1).all())
    net = m.net
    x = torch.randn(2, 3, 64, 96, device=DEV)
    with torch.no_grad():
        p2d, fg = net.inference_batch_images_seg_kp(x)
        assert torch.equal(fg, net.inference_batch_images_onlyseg(x)) and p2d.shape == (2, 7, 2)
        with pytest.raises(nv.HrpError, match="robot.*points_3d|points_3d.*robot"):
            net.inference_batch_images(x, torch.zeros(2, 7))
        # 3-D points built so that, under a known pose, they project exactly onto the key-points the network detects: the detected
        # pixels are lifted onto their rays of net.K at depths of their own and taken back through the pose.  The solver, fed the
        # detections, these points and net.K by the method under test, must return a pose that reprojects onto the detections (a
        # wrong K or a wrong argument order cannot).  The pose ITSELF is not gated here: a random network's key-points sit close
        # together, and seven near-coincident pixels fix a pose only loosely (measured: 3e-5 px of reprojection error next to 2e-2 of
        # pose error); how well the solver recovers a pose from well-spread points is pinned in tests/test_gpu_pnp.py (1e-5).
        g = torch.Generator().manual_seed(3)
        pose = torch.tensor([[0.2, -0.1, 0.3, 0.05, -0.02, 1.5], [-0.3, 0.2, 0.1, -0.04, 0.03, 1.8]], device=DEV)
        M = net.cTr_to_pose_matrix(pose)
        z = (torch.rand(2, 7, 1, generator=g) * 0.8 - 0.4).to(DEV) + pose[:, None, 5:6]
        ray = torch.cat([(p2d - net.K[:2, 2]) / torch.stack([net.K[0, 0], net.K[1, 1]]), torch.ones(2, 7, 1, device=DEV)], -1)
        pts = torch.einsum("bnj,bji->bni", ray * z - M[:, None, :3, 3], M[:, :3, :3])           # R^T (cam - t)
        cTr, p2, fg2 = net.inference_batch_images(x, None, points_3d=pts)
        assert cTr.shape == (2, 6) and torch.equal(p2, p2d) and torch.equal(fg2, fg)
        c1, p1, f1 = net.inference_single_image(x[0], None, points_3d=pts[0])
        assert c1.shape == (1, 6) and torch.equal(p1, p2d[:1])
        for got, b in ((cTr[0:1], 0), (cTr[1:2], 1), (c1, 0)):
            rep = batch_project(got, pts[b], net.K)[0]
            print(f"\nPnP stream {b}: reprojection error {(rep - p2d[b]).abs().max().item():.2e} px, pose error "
                  f"{(got[0] - pose[b]).abs().max().item():.2e}")
            assert (rep - p2d[b]).abs().max().item() < 0.05           # px of a 96 x 64 image; the solver's own tests hold 1e-2
            assert float(got[0, 5]) > 0                               # in front of the camera

        class Robot:                       # the caller's URDFRobot: only get_keypoints_only_fk is used
            def get_keypoints_only_fk(self, q):
                return pts[: q.shape[0]]
        net.robot = Robot()
        cR, _, _ = net.inference_batch_images(x, torch.zeros(2, 7))
        assert torch.equal(cR, cTr)
        proj = torch.stack([batch_project(pose[i:i + 1], pts[i], net.K)[0] for i in range(2)])
        cam = torch.einsum("bij,bnj->bni", M[:, :3, :3], pts) + M[:, None, :3, 3]
        uv = torch.einsum("ij,bnj->bni", net.K, cam)
        assert torch.allclose(uv[..., :2] / uv[..., 2:], proj, atol=1e-3)
        assert torch.equal(M[:, 3], torch.tensor([0.0, 0, 0, 1], device=DEV).expand(2, 4))
        R = net.to_valid_R_batch(M[:, :3, :3] + 0.01 * torch.randn(2, 3, 3, device=DEV))
        assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, device=DEV).expand(2, 3, 3), atol=1e-5)
