"""CPU checks of the back-propagatable PnP (lib/utils/BPnP.py): the golden_pnp.npz fixture, the package's
angle_axis_to_rotation_matrix against the reference's, a float64 host restatement of the reference's backward formula (the
formula csrc/pnp.hip implements; the GPU tests reuse it), and the C ABI declarations.

The host arithmetic here is element-wise products and sums only (no BLAS / LAPACK call): the small products and the 6 x 6 solve
are written out, so the checks depend on no vendor math library's dispatch."""
import os
import re

import numpy as np
import torch

from conftest import GOLDEN, ROOT

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv
from hrpe_amd.lib.utils.geometries import angle_axis_to_rotation_matrix


def load_pnp():
    return np.load(os.path.join(GOLDEN, "golden_pnp.npz"))


def rodrigues_np(w):
    """exact angle-axis -> rotation, float64, [B,3] -> [B,3,3]"""
    w = np.asarray(w, np.float64)
    out = np.zeros((w.shape[0], 3, 3))
    for i, v in enumerate(w):
        th = np.sqrt((v * v).sum())
        W = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        A = np.sin(th) / th if th > 1e-8 else 1.0 - th * th / 6
        B = (1 - np.cos(th)) / th ** 2 if th > 1e-8 else 0.5 - th * th / 24
        out[i] = np.eye(3) + A * W + B * np.einsum("ij,jk->ik", W, W)
    return out


def reproj_rms(P6d, X, x, K):
    """per-sample RMS reprojection error (px) of poses P6d [B,6] for points X [B,n,3] (or [n,3]), x [B,n,2]"""
    R = rodrigues_np(P6d[:, :3])
    X = np.broadcast_to(X, x.shape[:2] + (3,)).astype(np.float64)
    c = np.einsum("bij,bnj->bni", R, X) + P6d[:, None, 3:]
    p = np.einsum("bnj,ij->bni", c, np.asarray(K, np.float64))
    e = p[..., :2] / p[..., 2:3] - x
    return np.sqrt((e ** 2).sum(-1).mean(-1))


def solve_lu(A, b):
    """A x = b for a small square float64 tensor: Gaussian elimination with partial pivoting (the reference uses torch.inverse)"""
    A = A.detach().clone().double()
    x = b.detach().clone().double()
    m = A.shape[0]
    for k in range(m):
        p = k + int(torch.argmax(A[k:, k].abs()))
        if p != k:
            A[[k, p]] = A[[p, k]]
            x[[k, p]] = x[[p, k]]
        for r in range(k + 1, m):
            f = A[r, k] / A[k, k]
            A[r, k:] -= f * A[k, k:]
            x[r] -= f * x[k]
    for r in range(m - 1, -1, -1):
        x[r] = (x[r] - (A[r, r + 1:] * x[r + 1:]).sum()) / A[r, r]
    return x


def host_bpnp_backward(pts2d, pts3d, K, P6d, grad_output, fast=False):
    """The reference's BPnP / BPnP_m3d / BPnP_fast backward (BPnP.py:50-111, 154-236, 280-341) restated in float64 with torch
    autograd: f_j = sum_i coef_ij . r_i, r_i = x_i S_i - (K [R|t] z_i)_{0:2}, coef = -2 dpi/dy from get_coefs (:344-357) with
    create_graph (dropped when fast), grad = -g^T J_fy^-1 J_f(x, z, K).  Shared pts3d [n,3] sums grad_z over the batch; grad_K
    is always summed.  Returns numpy float64 (grad_x [B,n,2], grad_z, grad_K [3,3])."""
    f64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    pts2d, pts3d, K, P6d, g = f64(pts2d), f64(pts3d), f64(K), f64(P6d), f64(grad_output)
    shared = pts3d.dim() == 2
    B, n = pts2d.shape[0], pts2d.shape[1]
    gx, gz, gK = torch.zeros(B, n, 2, dtype=torch.float64), torch.zeros_like(pts3d), torch.zeros(3, 3, dtype=torch.float64)

    def project(y, z, k):              # y [n,6] rows, z [n,3] -> P [n,3]
        R = angle_axis_to_rotation_matrix(y[:, :3])[:, :3, :3]
        cam = (R * z[:, None, :]).sum(-1) + y[:, 3:]
        return (cam[:, None, :] * k[None]).sum(-1)

    with torch.enable_grad():
        for i in range(B):
            x = pts2d[i].clone().requires_grad_()
            y = P6d[i].clone().requires_grad_()
            z = (pts3d if shared else pts3d[i]).clone().requires_grad_()
            k = K.clone().requires_grad_()
            yr = y.unsqueeze(0).repeat(n, 1)
            P = project(yr, z, k)
            S = P[:, 2:3]
            r = x * S - P[:, :2]
            pi = P[:, :2] / S
            coefs = torch.stack([-2 * torch.autograd.grad(pi[:, c].sum(), yr, create_graph=not fast, retain_graph=True)[0]
                                 for c in range(2)], 1)          # [n, 2, 6]
            if fast:
                coefs = coefs.detach()
            Jy, Jx, Jz, JK = [], [], [], []
            for j in range(6):
                fj = (coefs[:, :, j] * r).sum()
                d = torch.autograd.grad(fj, (y, x, z, k), retain_graph=True, allow_unused=True)
                d = [torch.zeros_like(t) if dd is None else dd for dd, t in zip(d, (y, x, z, k))]
                Jy.append(d[0]); Jx.append(d[1].reshape(-1)); Jz.append(d[2].reshape(-1)); JK.append(d[3].reshape(-1))
            Jy, Jx, Jz, JK = (torch.stack(a) for a in (Jy, Jx, Jz, JK))
            v = solve_lu(Jy.t(), g[i])
            vT = lambda J: (v[:, None] * J).sum(0)  # noqa: E731
            gx[i] = -vT(Jx).view(n, 2)
            if shared:
                gz += -vT(Jz).view(n, 3)
            else:
                gz[i] = -vT(Jz).view(n, 3)
            gK += -vT(JK).view(3, 3)
    return gx.numpy(), gz.numpy(), gK.numpy()


def test_angle_axis_to_rotation_matrix_matches_reference():
    g = load_pnp()
    for c in g["cases"]:
        R = angle_axis_to_rotation_matrix(torch.tensor(g[f"{c}_P6d"][:, :3]))
        assert R.shape[1:] == (4, 4)
        np.testing.assert_allclose(R.numpy(), g[f"{c}_R_ref"], atol=1e-6, err_msg=str(c))
    R = angle_axis_to_rotation_matrix(torch.tensor(g["small_aa"]))
    np.testing.assert_allclose(R.numpy(), g["small_R_ref"], atol=1e-6)
    R = angle_axis_to_rotation_matrix(torch.tensor(g["small_aa"], dtype=torch.float64))
    np.testing.assert_allclose(R.numpy(), g["small_R_ref64"], atol=1e-12)
    # the fixture reaches both branches
    th2 = (g["small_aa"].astype(np.float64) ** 2).sum(1)
    assert (th2 <= 1e-6).sum() >= 3 and (th2 > 1e-6).sum() >= 2


def test_golden_pnp_fixture_consistent():
    g = load_pnp()
    assert os.path.getsize(os.path.join(GOLDEN, "golden_pnp.npz")) < 1 << 20
    assert list(g["cases"]) == ["panda_s0", "panda_s1", "panda_s3", "kuka_s1", "baxter_s1", "shared_s1"]
    for c in g["cases"]:
        x, X, K, P = g[f"{c}_pts2d"], g[f"{c}_pts3d"], g[f"{c}_K"], g[f"{c}_P6d"]
        B, n = x.shape[:2]
        assert X.shape == ((n, 3) if g[f"{c}_shared"] else (B, n, 3))
        # the optimum is a stationary point of the objective, no worse than the generating pose
        rms, rms_true = reproj_rms(P, X, x, K), reproj_rms(g[f"{c}_P6d_true"], X, x, K)
        assert (rms <= rms_true + 1e-9).all(), c
        if g[f"{c}_sigma"] == 0:
            np.testing.assert_allclose(P, g[f"{c}_P6d_true"], atol=2e-6)
            assert rms.max() < 1e-3
        # fp32 and fp64 reference backward agree to the fp32 noise floor
        for k in ("gx", "gz", "gK"):
            a, b = g[f"{c}_{k}32"], g[f"{c}_{k}64"]
            assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), (c, k)
            assert np.isfinite(b).all()


def test_host_restatement_reproduces_reference_fp64_gradients():
    g = load_pnp()
    for c in g["cases"]:
        gx, gz, gK = host_bpnp_backward(g[f"{c}_pts2d"], g[f"{c}_pts3d"], g[f"{c}_K"], g[f"{c}_P6d"], g[f"{c}_grad_output"])
        for name, a in (("gx", gx), ("gz", gz), ("gK", gK)):
            ref = g[f"{c}_{name}64"]
            err = np.abs(a - ref).max() / np.abs(ref).max()
            assert err < 1e-9, f"{c} {name}: {err}"


def test_pnp_abi_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "hrp.h")).read()
    for name in ("hrp_pnp_solve", "hrp_pnp_bwd"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in nv.PROTOTYPES
    assert len(nv.PROTOTYPES["hrp_pnp_solve"]) == 12 and len(nv.PROTOTYPES["hrp_pnp_bwd"]) == 17


def test_bpnp_module_surface():
    import inspect
    from hrpe_amd.lib.utils import BPnP as M
    for cls in (M.BPnP, M.BPnP_m3d, M.BPnP_fast):
        assert issubclass(cls, torch.autograd.Function)
        assert list(inspect.signature(cls.forward).parameters) == ["ctx", "pts2d", "pts3d", "K", "ini_pose"]
    assert callable(M.batch_project) and callable(M.batch_transform_3d)
