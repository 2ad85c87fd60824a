"""GPU checks of the robust PnP (hrp_pnp_solve_robust / hrp_pnp_bwd_masked through lib/utils/BPnP.py) against golden_pnp_robust.npz:
the consensus equals the planted inlier mask and the pose the optimum over it where pnp_solve is pulled away by the outliers, clean
input and refine_all give pnp_solve's answers, unusable points (flag or NaN) stay out, no consensus falls back to pnp_solve's bits,
the backward is the host restatement's on the inliers, results are bit-reproducible and graph-capturable, and CtRNet takes the robust
pose when asked."""
import numpy as np
import pytest
import torch

from test_gpu_pnp import _pose_errors, _t
from test_pnp_host import host_bpnp_backward, load_pnp
from test_pnp_minimal_host import HYPOTHESES, load_robust

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv
from hrpe_amd.lib.utils import BPnP as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = list(HYPOTHESES)


def _case(g, c):
    return _t(g[f"{c}_pts2d"]), _t(g[f"{c}_pts3d"]), _t(g[f"{c}_K"])


def _np(*ts):
    return [t.cpu().numpy().astype(np.float64) if t.dtype.is_floating_point else t.cpu().numpy() for t in ts]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _close(P, P_ref, what, tol=1e-5):
    ang, dt = _pose_errors(P, P_ref)
    print(f"{what}: rotation {ang.max():.2e} rad, translation {dt.max():.2e} m")
    assert ang.max() < tol and dt.max() < tol, f"{what}: rotation {ang.max():.2e} rad, translation {dt.max():.2e} m"


@pytest.mark.parametrize("c", CASES)
def test_consensus_and_pose(c):
    g = load_robust()
    x, X, K = _case(g, c)
    mask = g[f"{c}_mask"].astype(bool)
    P, inl, status, rms = _np(*M.pnp_solve_robust(x, X, K))
    assert np.array_equal(inl, mask), (c, inl, mask)
    _close(P, g[f"{c}_P6d"], c)
    assert (status[:, 0] & nv.PNP_NO_CONSENSUS == 0).all() and (status[:, 0] & nv.PNP_CONVERGED != 0).all(), status
    assert np.array_equal(status[:, 2], mask.sum(1)) and (status[:, 3] == HYPOTHESES[c]).all() and (status[:, 1] > 0).all(), status
    assert (rms < 2.0).all(), rms
    # the solver without consensus is pulled away by the outliers on the same input
    P0 = _np(M.pnp_solve(x, X, K)[0])[0]
    ang, dt = _pose_errors(P0, g[f"{c}_P6d"])
    assert (np.maximum(ang, dt) > 1e-3).all(), (c, ang, dt)


def test_clean_input_equals_pnp_solve():
    g = load_pnp()
    x, X, K = (_t(g[f"panda_s1_{k}"]) for k in ("pts2d", "pts3d", "K"))
    P, inl, status, _ = _np(*M.pnp_solve_robust(x, X, K, reproj_error=1e6))
    P0 = _np(M.pnp_solve(x, X, K)[0])[0]
    assert inl.all() and (status[:, 2] == 7).all() and (status[:, 0] & nv.PNP_NO_CONSENSUS == 0).all()
    _close(P, P0, "clean panda_s1 against pnp_solve")
    _close(P, g["panda_s1_P6d"], "clean panda_s1 against the fixture")


@pytest.mark.parametrize("c", CASES)
def test_refine_all_reaches_the_all_point_optimum(c):
    g = load_robust()
    x, X, K = _case(g, c)
    P, inl, status, _ = _np(*M.pnp_solve_robust(x, X, K, refine_all=True))
    _close(P, g[f"{c}_P6d_all"], c + " refine_all")
    assert (status[:, 0] & nv.PNP_NO_CONSENSUS == 0).all()


def test_valid_mask_and_nan_keypoint():
    g = load_robust()
    c = "baxter_s1"
    x, X, K = _case(g, c)
    mask = g[f"{c}_mask"].astype(bool)
    ref = M.pnp_solve_robust(x, X, K)
    # the planted outliers marked unusable: the same consensus, the same pose
    P, inl, status, _ = _np(*M.pnp_solve_robust(x, X, K, valid=torch.tensor(mask, device=DEV)))
    assert np.array_equal(inl, mask) and (status[:, 3] == 12 * 11 * 10 // 6).all(), status
    _close(P, g[f"{c}_P6d"], c + " valid")
    _close(P, _np(ref[0])[0], c + " valid against unmasked", tol=1e-6)
    # a NaN key-point in sample 2 (one of its outliers) behaves as unusable; the other samples keep their bits
    bad = int(np.flatnonzero(~mask[2])[0])
    xn = x.clone()
    xn[2, bad, 0] = float("nan")
    got = M.pnp_solve_robust(xn, X, K)
    keep = [i for i in range(x.shape[0]) if i != 2]
    for a, b in zip(got, ref):
        assert torch.equal(_bits(a)[keep], _bits(b)[keep])
    P, inl, status, rms = _np(*got)
    assert np.array_equal(inl[2], mask[2]) and status[2, 3] == 16 * 15 * 14 // 6 and np.isfinite(P).all() and np.isfinite(rms).all()
    _close(P[2:3], g[f"{c}_P6d"][2:3], c + " NaN key-point")
    # the same through a NaN 3-D coordinate
    Xn = X.clone()
    Xn[2, bad, 1] = float("nan")
    P2, inl2, _, _ = _np(*M.pnp_solve_robust(x, Xn, K))
    assert np.array_equal(inl2, mask) and np.array_equal(P2[2], P[2])


def test_fewer_than_four_usable_points():
    """A sample left with three usable points has no hypotheses: both flags are raised, no unusable point is reported as an inlier,
    the call returns, and the other samples keep their bits."""
    g = load_robust()
    x, X, K = _case(g, "kuka_s1")
    ref = M.pnp_solve_robust(x, X, K)
    valid = torch.ones(x.shape[:2], dtype=torch.bool, device=DEV)
    valid[3, 3:] = False
    got = M.pnp_solve_robust(x, X, K, valid=valid)
    keep = [i for i in range(x.shape[0]) if i != 3]
    for a, b in zip(got, ref):
        assert torch.equal(_bits(a)[keep], _bits(b)[keep])
    _, inl, status, _ = _np(*got)
    assert status[3, 0] & nv.PNP_FEW_POINTS and status[3, 0] & nv.PNP_NO_CONSENSUS and status[3, 3] == 0, status[3]
    assert not inl[3, 3:].any() and status[3, 2] == inl[3].sum()
    assert (status[keep, 0] & (nv.PNP_FEW_POINTS | nv.PNP_NO_CONSENSUS) == 0).all()


def test_no_consensus_falls_back_to_pnp_solve_bits():
    g = load_pnp()
    X, K = _t(g["panda_s0_pts3d"]), _t(g["panda_s0_K"])
    rng = np.random.Generator(np.random.PCG64(21))
    x = _t((rng.random((8, 7, 2)) * np.array([640.0, 480.0])).astype(np.float32))
    P, inl, status, rms = M.pnp_solve_robust(x, X, K, reproj_error=3.0)
    P0, st0, rms0 = M.pnp_solve(x, X, K)
    st = status.cpu().numpy()
    assert (st[:, 0] & nv.PNP_NO_CONSENSUS != 0).all() and (st[:, 3] == 35).all(), st
    assert torch.equal(_bits(P), _bits(P0)) and torch.equal(_bits(rms), _bits(rms0))
    assert np.array_equal(st[:, 1], st0.cpu().numpy()[:, 1])
    assert np.array_equal((st[:, 0] & nv.PNP_CONVERGED) != 0, st0.cpu().numpy()[:, 0] != 0)
    assert np.array_equal(st[:, 2], inl.cpu().numpy().sum(1))


def test_four_points():
    """The first four key-points of the noise-free panda_s0 (exact projections of the generating pose): four hypotheses, all four
    points inliers, and the generating pose recovered in every sample.  pnp_solve is compared where it is a reference: with four
    points its EPnP start can end LM in another local minimum of the objective (sample 4 of this fixture, 1.4 rad from the generating
    pose), so the two are held equal on the samples where pnp_solve itself reaches the generating pose, at least six of the eight."""
    g = load_pnp()
    x, X, K = (_t(g[f"panda_s0_{k}"]) for k in ("pts2d", "pts3d", "K"))
    x, X = x[:, :4].contiguous(), X[:, :4].contiguous()
    P, inl, status, _ = _np(*M.pnp_solve_robust(x, X, K))
    P0 = _np(M.pnp_solve(x, X, K)[0])[0]
    assert inl.all() and (status[:, 2] == 4).all() and (status[:, 3] == 4).all() and (status[:, 0] & nv.PNP_NO_CONSENSUS == 0).all()
    _close(P, g["panda_s0_P6d_true"], "n = 4 against the generating pose")
    ang, dt = _pose_errors(P0, g["panda_s0_P6d_true"])
    good = np.maximum(ang, dt) < 1e-5
    print("pnp_solve reaches the generating pose from four points in samples", np.flatnonzero(good))
    assert good.sum() >= 6
    _close(P[good], P0[good], "n = 4 against pnp_solve")


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_backward_on_the_inliers():
    """BPnP_robust's gradients against the host restatement evaluated on each sample's inlier subset (at the device's pose, fp64), the
    outliers' rows exactly zero; per-sample pts3d (kuka_s1) and, for the shared form, one sample's points for the whole batch."""
    g = load_robust()
    c = "kuka_s1"
    mask = g[f"{c}_mask"].astype(bool)
    x, X, K = _case(g, c)
    go = np.random.Generator(np.random.PCG64(7)).normal(size=(x.shape[0], 6)).astype(np.float32)
    x.requires_grad_(); X.requires_grad_(); K.requires_grad_()
    P, inl = M.BPnP_robust.apply(x, X, K, 3.0)
    assert np.array_equal(inl.cpu().numpy(), mask) and not inl.requires_grad
    P.backward(_t(go))
    gx, gz, gK = _np(x.grad, X.grad, K.grad)
    Pd = P.detach().cpu().numpy().astype(np.float64)
    hx, hz, hK = np.zeros_like(gx), np.zeros_like(gz), np.zeros((3, 3))
    for i in range(x.shape[0]):
        m = mask[i]
        a, b, k = host_bpnp_backward(g[f"{c}_pts2d"][i:i + 1, m], g[f"{c}_pts3d"][i:i + 1, m], g[f"{c}_K"], Pd[i:i + 1], go[i:i + 1])
        hx[i, m], hz[i, m] = a[0], b[0]
        hK += k
    for what, a, b in (("grad_x", gx, hx), ("grad_z", gz, hz), ("grad_K", gK, hK)):
        print(f"{c} {what}: {_rel(a, b):.2e}")
        assert _rel(a, b) <= 1e-4, (what, _rel(a, b))
    assert (gx[~mask] == 0).all() and (gz[~mask] == 0).all() and (np.abs(gx[mask]).max(-1) > 0).all()
    # shared pts3d [n, 3]: sample 0's points and key-points for two views
    xs, Xs = _t(g[f"{c}_pts2d"][:1].repeat(2, 0)), _t(g[f"{c}_pts3d"][0])
    xs.requires_grad_(); Xs.requires_grad_()
    Ps, _ = M.BPnP_robust.apply(xs, Xs, K.detach(), 3.0)
    Ps.backward(_t(go[:2]))
    m = mask[0]
    a, b, _ = host_bpnp_backward(g[f"{c}_pts2d"][:1].repeat(2, 0)[:, m], g[f"{c}_pts3d"][0][m], g[f"{c}_K"],
                                 Ps.detach().cpu().numpy().astype(np.float64), go[:2])
    assert _rel(_np(xs.grad)[0][:, m], a) <= 1e-4 and _rel(_np(Xs.grad)[0][m], b) <= 1e-4
    assert (_np(Xs.grad)[0][~m] == 0).all()


def test_backward_refine_all_is_the_fast_backward_over_all_points():
    g = load_robust()
    c = "panda_s0"
    x, X, K = _case(g, c)
    go = np.random.Generator(np.random.PCG64(8)).normal(size=(x.shape[0], 6)).astype(np.float32)
    x.requires_grad_(); X.requires_grad_(); K.requires_grad_()
    P, _ = M.BPnP_robust.apply(x, X, K, 3.0, True)
    P.backward(_t(go))
    host = host_bpnp_backward(g[f"{c}_pts2d"], g[f"{c}_pts3d"], g[f"{c}_K"], P.detach().cpu().numpy().astype(np.float64), go, fast=True)
    for what, a, b in zip(("grad_x", "grad_z", "grad_K"), _np(x.grad, X.grad, K.grad), host):
        print(f"{c} refine_all {what}: {_rel(a, b):.2e}")
        assert _rel(a, b) <= 1e-4, (what, _rel(a, b))


def test_bit_reproducible_and_permutation_equivariant():
    g = load_robust()
    for c in ("panda_s0", "cloud24"):
        x, X, K = _case(g, c)
        a, b = M.pnp_solve_robust(x, X, K), M.pnp_solve_robust(x, X, K)
        for u, v in zip(a, b):
            assert torch.equal(_bits(u), _bits(v))
        perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], device=DEV)
        p = M.pnp_solve_robust(x[perm].contiguous(), X[perm].contiguous(), K)
        for u, v in zip(a, p):
            assert torch.equal(_bits(u)[perm], _bits(v))


def test_graph_capture():
    g = load_robust()
    x, X, K = _case(g, "baxter_s1")
    eager = M.pnp_solve_robust(x, X, K)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        M.pnp_solve_robust(x, X, K)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M.pnp_solve_robust(x, X, K)
    graph.replay()
    torch.cuda.synchronize()
    for u, v in zip(out, eager):
        assert torch.equal(_bits(u), _bits(v))


def test_ctrnet_takes_the_robust_pose_when_asked():
    from hrpe_amd.lib.models.ctrnet.CtRNet import CtRNet
    g = load_robust()
    c = "panda_s0"
    x, X, K = _case(g, c)
    net = CtRNet.__new__(CtRNet)
    torch.nn.Module.__init__(net)
    net.K = K
    seg = torch.zeros(x.shape[0], 1, 4, 4, device=DEV)
    net._seg_kp = lambda img: (x[: img.shape[0]], seg[: img.shape[0]])
    img = torch.zeros(x.shape[0], 3, 4, 4, device=DEV)
    cTr, p2d, fg = net.inference_batch_images(img, None, points_3d=X, reproj_error=3.0)
    want = M.pnp_solve_robust(x, X, K)
    assert torch.equal(cTr, want[0]) and torch.equal(net.last_inliers, want[1]) and torch.equal(p2d, x) and fg.shape == seg.shape
    assert np.array_equal(net.last_inliers.cpu().numpy(), g[f"{c}_mask"].astype(bool))
    plain, _, _ = net.inference_batch_images(img, None, points_3d=X)
    assert torch.equal(plain, M.pnp_solve(x, X, K)[0]) and not torch.equal(plain, cTr)
    one, _, _ = net.inference_single_image(img[0], None, points_3d=X[0], reproj_error=3.0)
    assert torch.equal(one, want[0][:1]) and torch.equal(net.last_inliers, want[1][:1])
    one_plain, _, _ = net.inference_single_image(img[0], None, points_3d=X[0])
    assert torch.equal(one_plain, M.pnp_solve(x[:1], X[0], K)[0])
