"""The float64 oracle of the pose-head kernels (tests/heads_oracle.py) proved on the CPU: against the fp32 oracle of oracle/heads.py
and oracle/fk.py, which the reference's own fixtures pin, and against those fixtures directly.  No GPU, no call into the library: the
chain descriptors come from parse_chain, which only reads the URDF.  The GPU tests (test_gpu_heads.py) then compare the kernels with
this oracle."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hrpe_amd  # noqa: F401
from conftest import GOLDEN, PANDA_URDF
from hrpe_amd.lib.dataset.const import MESH_LINKS
from hrpe_amd.lib.utils.urdf_robot import URDFRobot, parse_chain
from oracle import fk, heads

import heads_oracle as O
from heads_oracle import F32, F64

URDF = {r: os.path.join(os.path.dirname(PANDA_URDF), f"{r}_kinematics.urdf") for r in ("panda", "kuka", "baxter")}
FULL_YAML = [1.0, 1.0, 1.0, 10.0, 1.0, 10.0, 10.0, 10.0, 10.0, 0.0]     # pose rot uv depth trans kp2d kp3d kp2d_int kp3d_int align


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def test_softargmax3d_matches_oracle_and_fixture():
    g = load("golden_integral.npz")
    rng = np.random.Generator(np.random.PCG64(int(g["seed"])))
    out = torch.as_tensor(rng.normal(0, 2.0, (2, 7 * 64, 64, 64)).astype(np.float32))
    out[:, ::5] += 3.0
    uvd, ms = O.softargmax3d(nhwc(out), 7, 64, root=3, fix_root=1)
    np.testing.assert_allclose(uvd.numpy(), g["uvd"], atol=1e-6)                              # the fixture's tolerance
    np.testing.assert_allclose(uvd.numpy(), heads.soft_argmax_uvd(out).numpy(), atol=1e-6)
    free, _ = O.softargmax3d(nhwc(out), 7, 64, root=3, fix_root=0)
    np.testing.assert_allclose(free.numpy(), heads.soft_argmax_uvd(out, fix_root=False).numpy(), atol=1e-6)
    x = out.double().reshape(2, 7, -1)
    assert torch.equal(ms[..., 0], x.amax(2))
    np.testing.assert_allclose(ms[..., 1].numpy(), torch.exp(x - x.amax(2, keepdim=True)).sum(2).numpy(), rtol=1e-13)


def test_softargmax3d_small_odd_shape_and_fp32_form():
    """H != W, D != H, the pixel / depth split of the channel-last layout; the fp32 form (exp2 of the rounded product) is the same
    function to fp32 accuracy."""
    gen = torch.Generator().manual_seed(11)
    B, J, D, H, W = 2, 3, 4, 5, 7
    out = 2.0 * torch.randn(B, J * D, H, W, generator=gen)
    p = F.softmax(out.double().reshape(B, J, -1), dim=2).reshape(B, J, D, H, W)      # integral.py:147-177 with three sizes
    ar = lambda n: torch.arange(n, dtype=F64)                                        # noqa: E731
    ref = torch.stack(((p.sum((2, 3)) * ar(W)).sum(2) / W - 0.5, (p.sum((2, 4)) * ar(H)).sum(2) / H - 0.5,
                       (p.sum((3, 4)) * ar(D)).sum(2) / D - 0.5), 2)
    ref[:, 1, 2] = 0.0
    uvd, _ = O.softargmax3d(nhwc(out), J, D, root=1, fix_root=1)
    np.testing.assert_allclose(uvd.numpy(), ref.numpy(), atol=1e-13)
    u32, m32 = O.softargmax3d(nhwc(out), J, D, root=1, fix_root=1, dt=F32)
    assert u32.dtype == F32 and float((u32.double() - uvd).abs().max()) < 1e-6


def test_softargmax_flat_matches_softmax():
    gen = torch.Generator().manual_seed(12)
    x = 3.0 * torch.randn(2, 65, 5, generator=gen, dtype=F64)
    coord, ms = O.softargmax_flat(x)
    p = F.softmax(x, 1)
    np.testing.assert_allclose(coord.numpy(), ((p * torch.arange(65.0, dtype=F64)[None, :, None]).sum(1) / 65).numpy(), atol=1e-14)
    assert torch.equal(ms[..., 0], x.amax(1))
    one, _ = O.softargmax_flat(x[:, :1])
    assert float(one.abs().max()) == 0.0


def test_pose_geometry_matches_oracle():
    gen = torch.Generator().manual_seed(13)
    B, J, root = 5, 7, 3
    uvd = torch.rand(B, J, 3, generator=gen) - 0.5
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1] = 400 + 50 * torch.rand(B, generator=gen), 350 + 50 * torch.rand(B, generator=gen)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 120 + 10 * torch.rand(B, generator=gen), 131.0, 1.0
    gamma, kval = 1.0 + torch.rand(B, generator=gen), 900 + 200 * torch.rand(B, generator=gen)
    depth, xyz, ruv, trans = O.pose_geometry(gamma, kval, uvd, K, root, 256.0, 1.3)
    z = (gamma * kval / 1000.0).view(B, 1)
    np.testing.assert_allclose(depth.numpy(), z[:, 0].numpy(), rtol=1e-6)
    np.testing.assert_allclose(xyz.numpy(), heads.uvd_to_xyz(uvd, K, z).numpy(), atol=2e-6)
    ruv_ref = (uvd[:, root, :2] + 0.5) * 256.0
    np.testing.assert_allclose(ruv.numpy(), ruv_ref.numpy(), atol=1e-4)
    np.testing.assert_allclose(trans.numpy(), heads.uvz2xyz_singlepoint(ruv_ref, z, K).numpy(), atol=2e-6)


def _uv_ok(uv, ref_uv, ref_xyz):
    """test_gpu_kernels._check_uv: 1e-3 px at a working distance, 2e-4 relative everywhere."""
    sane = (ref_xyz[..., 2] > 0.5) & (np.abs(ref_uv).max(-1) < 512)
    assert sane.mean() > 0.3
    assert np.abs(uv - ref_uv)[sane].max() < 1e-3
    assert (np.abs(uv - ref_uv) / (np.abs(ref_uv) + 1.0)).max() < 2e-4


@pytest.mark.parametrize("robot_type", ["panda", "kuka", "baxter"])
def test_fk_interpreter_reproduces_reference_fixtures(robot_type):
    """The chain interpreter on parse_chain's descriptors against golden_fk*.npz at the tolerances of test_fk_golden /
    test_fk_golden_other_robots (tests/test_gpu_kernels.py)."""
    g = load("golden_fk.npz" if robot_type == "panda" else f"golden_fk_{robot_type}.npz")
    chain = URDFRobot(robot_type, urdf_path=URDF[robot_type]).chain
    q, r, t, K = [torch.tensor(g[k]) for k in ("q", "rot6d", "t", "K")]
    B = q.shape[0]
    assert chain.dof == q.shape[1] and chain.nkp == g["fk_only"].shape[1]
    eye = torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(B, 1)
    only, _, _ = O.fk(chain, q, eye, torch.zeros(B, 3))
    np.testing.assert_allclose(only.numpy(), g["fk_only"], atol=2e-6 if robot_type == "panda" else 3e-6)
    wx, wu = torch.tensor(g["w_xyz"]), torch.tensor(g["w_uv"])
    for root in g["roots"].tolist():
        xyz, uv, rr = O.fk(chain, q, r, t, K, root)
        np.testing.assert_allclose(xyz.numpy(), g[f"xyz_root{root}"], atol=3e-6 if robot_type == "panda" else 5e-6)
        _uv_ok(uv.numpy(), g[f"uv_root{root}"], g[f"xyz_root{root}"])
        if root:
            np.testing.assert_allclose(rr.numpy(), g[f"rootrot_root{root}"], atol=3e-6)
        else:       # the reference hands its input back at root 0 (urdf_robot.py:113-117); the kernel writes the matrix rows
            assert np.array_equal(g["rootrot_root0"], g["rot6d"])
            np.testing.assert_allclose(rr.numpy(), fk.rot6d_to_rotmat(r.double())[:, :2].reshape(B, 6).numpy(), atol=1e-15)
        grads = O.vjp(lambda a, b, c: O.fk(chain, a, b, c, K, root)[:2], (q, r, t), (wx, wu))
        for name, got in zip(("gq", "grot", "gt"), grads):
            ref = g[f"{name}_root{root}"]
            np.testing.assert_allclose(got.numpy(), ref, atol=3e-4 * max(1.0, np.abs(ref).max()), rtol=2e-3, err_msg=name)


def test_fk_quaternion_fixture():
    g = load("golden_fk_quat.npz")
    chain = URDFRobot("panda", urdf_path=URDF["panda"]).chain
    q, r, t, K = [torch.tensor(g[k]) for k in ("q", "rot6d", "t", "K")]
    assert r.shape[1] == 4
    for root in (0, 3):
        xyz, uv, rr = O.fk(chain, q, r, t, K, root)
        np.testing.assert_allclose(xyz.numpy(), g[f"xyz_root{root}"], atol=3e-6)
        if root:        # the tolerance of test_fk_kernel_with_quaternion_rotation_golden: the fixture holds samples with w = 0.02
            ref = g[f"rootrot_root{root}"]
            tol = 3e-6 + 1e-6 / np.maximum(np.abs(ref[:, :1]), 1e-3)
            assert (np.abs(rr.numpy() - ref) <= tol).all(), float((np.abs(rr.numpy() - ref) / tol).max())


@pytest.mark.parametrize("damped", [False, True])
def test_pose_loss_matches_full_loss(damped):
    """full.yaml's weights on the inputs of test_fused_pose_loss_matches_tensor_expressions: terms, total and every gradient."""
    pred, gt, K, uvd = O.pose_loss_inputs(5 + int(damped), 37, damped)
    out = O.pose_loss(pred, gt, K, FULL_YAML, 3, 256.0)
    leaves = [p.clone().requires_grad_(True) for p in pred]
    loss, terms = heads.full_loss(leaves[:5] + [uvd] + leaves[5:], gt, K)
    assert (float(torch.norm(pred[2] - gt["root_trans"], dim=1).mean()) > 0.5) == damped
    for k, n in enumerate(O.TERMS):
        np.testing.assert_allclose(float(out[k]), float(terms[n].detach()), rtol=2e-6, err_msg=n)
    np.testing.assert_allclose(float(out[10]), float(loss.detach()), rtol=2e-6)
    loss.backward()
    grads = O.vjp(lambda *p: (O.pose_loss(p, gt, K, FULL_YAML, 3, 256.0)[10],), pred, (torch.ones(()),))
    for n, got, leaf in zip(O.PRED, grads, leaves):
        np.testing.assert_allclose(got.numpy(), leaf.grad.numpy(), rtol=2e-5, atol=2e-7 * float(leaf.grad.abs().max()), err_msg=n)


def test_pose_loss_weight_order():
    """Each of the ten weights multiplies its own term: with weight k alone set to 1 the total is the term TERM_WEIGHT maps to it."""
    pred, gt, K, _ = O.pose_loss_inputs(3, 4, False)
    for k in range(10):
        w = [0.0] * 10
        w[k] = 1.0
        out = O.pose_loss(pred, gt, K, w, 3, 256.0)
        assert float(out[10]) == float(out[O.TERM_WEIGHT.index(k)]) and float(out[10]) > 0
    names = dict(zip(O.TERM_WEIGHT, O.TERMS))
    assert names[5] == "loss_error2d" and names[6] == "loss_error3d" and names[7] == "loss_error2d_int" and names[8] == "loss_error3d_int"


def test_mesh_pose_matches_oracle():
    """The panda mesh chain at roots 0 and 3 on the fixture's inputs (samples 3 and 7 are behind the camera)."""
    g = load("golden_mesh_pose.npz")
    robot = fk.Robot(PANDA_URDF)
    mine = URDFRobot("panda", urdf_path=URDF["panda"])
    names = MESH_LINKS["panda"]
    chain, _ = parse_chain(URDF["panda"], names)
    q, r6, t = torch.tensor(g["q"]), torch.tensor(g["rot6d"]), torch.tensor(g["t"])
    verts, vl = torch.tensor(g["verts"]), torch.tensor(g["vert_link"])
    for root in (0, 3):
        root_kp = names.index(mine.link_names[root]) if root else -1
        xyz, _, s = O.mesh_pose(chain, q, r6, t, root_kp, verts, vl)
        np.testing.assert_allclose(xyz.numpy(), fk.pose_mesh(robot, q, r6, t, verts, vl, root=root).numpy(), atol=5e-6)
        np.testing.assert_allclose(xyz.numpy(), g[f"cam_root{root}"], atol=5e-6)
        assert s[3] == -1 and s[7] == -1 and (xyz[[3, 7], :, 2].mean(1) > 0).all()


def test_rot6d_compose_project_l1():
    gen = torch.Generator().manual_seed(14)
    a, b = torch.randn(5, 6, generator=gen, dtype=F64), torch.randn(5, 6, generator=gen, dtype=F64)
    R = fk.rot6d_to_rotmat(a) @ fk.rot6d_to_rotmat(b)
    assert torch.equal(O.rot6d_compose(a, b), R[:, :2].reshape(5, 6))
    np.testing.assert_allclose((R @ R.transpose(1, 2)).numpy(), np.broadcast_to(np.eye(3), (5, 3, 3)), atol=1e-14)
    K, p = torch.randn(2, 3, 3, generator=gen, dtype=F64), torch.randn(2, 4, 3, generator=gen, dtype=F64)
    h = (K[:, None] @ p[..., None])[..., 0]
    np.testing.assert_allclose(O.project(K, p).numpy(), (h[..., :2] / h[..., 2:]).numpy(), rtol=1e-14)
    pred, gtv = torch.tensor([1024.0, 3.0, -5.0]), torch.tensor([O.f32(1024.0 * np.float32(1e-3)), 0.0, 1.0])
    (gp,) = O.vjp(lambda x: (O.l1_loss(x, gtv, 1e-3),), (pred,), (torch.ones(()),))
    s = O.f32(1e-3)
    np.testing.assert_allclose(gp.numpy(), [0.0, s / 3, -s / 3], rtol=1e-15)
    np.testing.assert_allclose(float(O.l1_loss(pred, gtv, 1e-3)), (abs(3 * s) + abs(-5 * s - 1)) / 3, rtol=1e-15)
