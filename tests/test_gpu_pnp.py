"""GPU checks of the back-propagatable PnP (csrc/pnp.hip through lib/utils/BPnP.py) against golden_pnp.npz: the forward reaches the
objective's optimum from EPnP and from an initial pose, the backward matches the reference's own fp64 gradients, BPnP_fast the host
restatement without the coefficient derivatives, gradients flow through the FK to the joint angles, results are bit-reproducible and
graph-capturable, and prepare_batch(synthetic=False) builds a real-dataset batch."""
import numpy as np
import pytest
import torch

from conftest import PANDA_URDF
from test_pnp_host import host_bpnp_backward, load_pnp, reproj_rms, rodrigues_np

import hrpe_amd  # noqa: F401
from hrpe_amd.lib.utils import BPnP as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.tensor(np.asarray(a, np.float32), device=DEV)


def _case(g, c):
    return _t(g[f"{c}_pts2d"]), _t(g[f"{c}_pts3d"]), _t(g[f"{c}_K"])


def _pose_errors(P, P_ref):
    R, Rr = rodrigues_np(P[:, :3]), rodrigues_np(P_ref[:, :3])
    cosang = np.clip((np.trace(np.einsum("bji,bjk->bik", R, Rr), axis1=1, axis2=2) - 1) / 2, -1, 1)
    # arccos loses digits near 0: the angle from the skew part instead
    D = np.einsum("bji,bjk->bik", R, Rr)
    s = np.sqrt((np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], 1) ** 2).sum(1)) / 2
    ang = np.arctan2(s, cosang)
    return ang, np.abs(P[:, 3:] - P_ref[:, 3:]).max(1)


@pytest.mark.parametrize("with_init", [False, True])
def test_forward_reaches_optimum(with_init):
    g = load_pnp()
    for c in g["cases"]:
        x, X, K = _case(g, c)
        P_ref = g[f"{c}_P6d"]
        ini = None
        if with_init:
            rng = np.random.Generator(np.random.PCG64(5))
            ini = _t(P_ref + rng.normal(0, 0.02, P_ref.shape))
        P, status, rms = M.pnp_solve(x, X, K, ini)
        P, status, rms = P.cpu().numpy().astype(np.float64), status.cpu().numpy(), rms.cpu().numpy()
        assert (np.sqrt((P[:, :3] ** 2).sum(1)) <= np.pi + 1e-6).all()
        ang, dt = _pose_errors(P, P_ref)
        assert ang.max() < 1e-5 and dt.max() < 1e-5, f"{c}: rotation {ang.max():.2e} rad, translation {dt.max():.2e} m"
        rms_ref = reproj_rms(P_ref, g[f"{c}_pts3d"], g[f"{c}_pts2d"], g[f"{c}_K"])
        assert np.abs(rms - rms_ref).max() < 1e-4, (c, rms, rms_ref)
        assert (status[:, 0] == 1).all() and (status[:, 1] > 0).all(), (c, status)


def _grad_check(c, got, ref, ref32, what):
    err = np.abs(got - ref).max() / np.abs(ref).max()
    floor = np.abs(ref32 - ref).max() / np.abs(ref).max()
    print(f"{c} {what}: kernel {err:.2e}, fp32 reference {floor:.2e} (relative to max |fp64 reference|)")
    assert err <= 1e-4, f"{c} {what}: {err:.2e}"


def test_backward_matches_reference_fp64():
    g = load_pnp()
    for c in g["cases"]:
        shared = bool(g[f"{c}_shared"])
        x, X, K = _case(g, c)
        x.requires_grad_(); X.requires_grad_(); K.requires_grad_()
        fn = M.BPnP if shared else M.BPnP_m3d
        P = fn.apply(x, X, K)
        P.backward(_t(g[f"{c}_grad_output"]))
        # the backward evaluated at the fixture's optimum too (the forward's fp32 output differs from it in the last bits)
        gx, gz, gK, st = M.pnp_backward(x.detach(), X.detach(), K.detach(), _t(g[f"{c}_P6d"]), _t(g[f"{c}_grad_output"]))
        assert (st.cpu().numpy() == 0).all()
        for what, a, b in (("grad_x", x.grad, gx), ("grad_z", X.grad, gz), ("grad_K", K.grad, gK)):
            key = {"grad_x": "gx", "grad_z": "gz", "grad_K": "gK"}[what]
            ref, ref32 = g[f"{c}_{key}64"], g[f"{c}_{key}32"]
            assert tuple(a.shape) == ref.shape
            _grad_check(c, a.cpu().numpy(), ref, ref32, what + " (autograd)")
            _grad_check(c, b.cpu().numpy(), ref, ref32, what)


def test_backward_fast_matches_host_restatement():
    g = load_pnp()
    c = "shared_s1"
    x, X, K = _case(g, c)
    x.requires_grad_(); X.requires_grad_(); K.requires_grad_()
    P = M.BPnP_fast.apply(x, X, K)
    P.backward(_t(g[f"{c}_grad_output"]))
    host = host_bpnp_backward(g[f"{c}_pts2d"], g[f"{c}_pts3d"], g[f"{c}_K"], P.detach().cpu().numpy().astype(np.float64),
                              g[f"{c}_grad_output"], fast=True)
    full = host_bpnp_backward(g[f"{c}_pts2d"], g[f"{c}_pts3d"], g[f"{c}_K"], P.detach().cpu().numpy().astype(np.float64),
                              g[f"{c}_grad_output"], fast=False)
    for a, b, f in zip((x.grad, X.grad, K.grad), host, full):
        a = a.cpu().numpy()
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max()
        assert np.abs(b - f).max() > 1e-3 * np.abs(f).max()     # the dropped terms matter at sigma = 1


def test_end_to_end_gradient_through_fk_to_joint_angles():
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    from oracle import fk as ofk
    g = load_pnp()
    c = "panda_s1"
    robot = URDFRobot("panda")
    q = _t(g[f"{c}_q"]).requires_grad_()
    x, _, K = _case(g, c)
    X = robot.get_keypoints_only_fk(q)
    P = M.BPnP_m3d.apply(x, X, K)
    w = torch.tensor(np.random.Generator(np.random.PCG64(3)).normal(size=(x.shape[0], 6)), dtype=torch.float32, device=DEV)
    (P * w).sum().backward()
    # host: the restated backward at the device's optimum, composed with the FK oracle in float64
    orob = ofk.Robot(PANDA_URDF)
    qh = torch.tensor(g[f"{c}_q"], dtype=torch.float64, requires_grad=True)
    Xh = orob.get_keypoints_only_fk(qh)
    _, gz, _ = host_bpnp_backward(g[f"{c}_pts2d"], Xh.detach().numpy(), g[f"{c}_K"], P.detach().cpu().numpy().astype(np.float64),
                                  w.cpu().numpy())
    (Xh * torch.tensor(gz)).sum().backward()
    ref = qh.grad.numpy()
    err = np.abs(q.grad.cpu().numpy() - ref).max() / np.abs(ref).max()
    assert err < 1e-3, err


def test_bit_reproducible_and_graph_capturable():
    g = load_pnp()
    c = "baxter_s1"
    x, X, K = _case(g, c)
    go = _t(g[f"{c}_grad_output"])

    def run():
        P, st, rms = M.pnp_solve(x, X, K)
        gx, gz, gK, st2 = M.pnp_backward(x, X, K, P, go)
        return [P, st, rms, gx, gz, gK, st2]

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    for u, v in zip(out, a):
        assert torch.equal(u, v)


def _real_batch(robot, B, rotation_seed=0):
    """a DreamDataset-shaped batch whose keypoints_2d_original are exact projections of the FK key-points under TCO"""
    from hrpe_amd.lib.dataset.const import JOINT_BOUNDS, JOINT_NAMES
    rng = np.random.Generator(np.random.PCG64(rotation_seed))
    b = np.array(JOINT_BOUNDS["panda"])
    q = (b[:, 0] + (b[:, 1] - b[:, 0]) * rng.random((B, len(b)))).astype(np.float32)
    X = robot.get_keypoints_only_fk(torch.tensor(q, device=DEV)).double().cpu().numpy()
    ax = rng.normal(size=(B, 3))
    ax /= np.sqrt((ax ** 2).sum(1, keepdims=True))
    R = rodrigues_np(ax * rng.uniform(0.3, 2.5, (B, 1)))
    TCO = np.tile(np.eye(4), (B, 1, 1))
    TCO[:, :3, :3] = R
    TCO[:, :3, 3] = np.array([0.0, 0.0, 1.6]) - np.einsum("bij,bj->bi", R, X.mean(1))
    TCO = TCO.astype(np.float32)
    K = np.array([[615.0, 0, 320], [0, 615.0, 240], [0, 0, 1]], np.float32)
    cam = np.einsum("bij,bnj->bni", TCO[:, :3, :3].astype(np.float64), X) + TCO[:, None, :3, 3]
    p = np.einsum("bnj,ij->bni", cam, K.astype(np.float64))
    kp2d_orig = (p[..., :2] / p[..., 2:3]).astype(np.float32)
    n = X.shape[1]
    img = torch.zeros(B, 3, 8, 8, dtype=torch.uint8)
    bbox = torch.tensor([[10.0, 12.0, 200.0, 230.0]] * B)
    Kt = torch.tensor(K).repeat(B, 1, 1)
    return {"root": {"images": img, "K": Kt, "bbox_strict_bounded": bbox, "bbox_gt2d_extended": bbox},
            "other": {"images": img, "K": Kt, "keypoints_2d": torch.tensor(kp2d_orig) * 0.5,
                      "valid_mask_crop": torch.ones(B, n), "keypoints_3d": torch.tensor(cam.astype(np.float32))},
            "TCO": torch.tensor(TCO), "K_original": Kt, "keypoints_2d_original": torch.tensor(kp2d_orig),
            "jointpose": {nm: [float(q[i, j]) for i in range(B)] for j, nm in enumerate(JOINT_NAMES["panda"])}}


@pytest.mark.parametrize("rotation_dim", [6, 4])
def test_prepare_batch_real_dataset(rotation_dim):
    from hrpe_amd.lib.core.function import prepare_batch
    from hrpe_amd.lib.utils.geometries import rotmat_to_quat, rotmat_to_rot6d
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    robot = URDFRobot("panda")
    batch = _real_batch(robot, 8)
    real = prepare_batch(batch, robot, DEV, reference_keypoint_id=3, synthetic=False, rotation_dim=rotation_dim)
    syn = prepare_batch(batch, robot, DEV, reference_keypoint_id=3, synthetic=True, rotation_dim=rotation_dim)
    TCO = torch.as_tensor(batch["TCO"]).to(DEV)
    want = (rotmat_to_rot6d if rotation_dim == 6 else rotmat_to_quat)(TCO[:, :3, :3])
    assert (real["gt"]["rot"] - want).abs().max().item() < 1e-5
    for k, v in syn["gt"].items():
        if k in ("rot", "root_rot"):
            continue
        assert torch.equal(real["gt"][k], v), k
    for k in ("reg_images", "root_images", "root_K", "other_K", "k_values"):
        assert torch.equal(real[k], syn[k]), k
    assert (real["gt"]["root_rot"] - syn["gt"]["root_rot"]).abs().max().item() < 1e-4


def test_prepare_batch_real_dataset_feeds_full_loss():
    from hrpe_amd.lib.core.function import full_loss, prepare_batch
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    robot = URDFRobot("panda")
    batch = _real_batch(robot, 2, rotation_seed=1)
    b = prepare_batch(batch, robot, DEV, reference_keypoint_id=3, synthetic=False)
    gt = b["gt"]
    B = 2
    pred = (gt["pose"] + 0.01, gt["root_rot"] + 0.01, gt["trans"], gt["root_uv"] + 1.0, gt["root_depth"] * 1000.0,
            gt["kp2d"].new_zeros(B, 7, 3) + gt["root_trans"][:, None], gt["kp3d"] + 0.01, gt["kp3d"])
    for p in pred:
        p.requires_grad_()
    loss, terms = full_loss(pred, gt, b["other_K"])
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(v) for v in terms.values())


def test_rejects_bad_inputs():
    g = load_pnp()
    x, X, K = _case(g, "panda_s1")
    with pytest.raises(ValueError):
        M.BPnP_m3d.apply(x[:, :3], X[:, :3], K)
    with pytest.raises(ValueError):
        M.BPnP_m3d.apply(x.cpu(), X.cpu(), K.cpu())
    with pytest.raises(ValueError):
        M.BPnP.apply(x, X, K)          # BPnP needs pts3d [n, 3]
