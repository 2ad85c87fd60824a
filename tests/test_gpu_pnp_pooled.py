"""GPU checks of the pooled robust PnP (hrp_pnp_solve_pooled through lib/utils/BPnP.pnp_solve_pooled) and of what stands on it
(lib/core/calibrate.CameraCalibrator, CtRNet.inference_sequence): golden_pnp_pooled.npz's sequences end on the planted mask and the
float64 optimum over it, the robust solver's fixture gives the robust solver's consensus, the sizes at which the layout changes (one
wave, one workgroup stride, the largest n) recover a planted pose, problems of one call do not see each other, unusable points stay
out, the covariance is s^2 (J^T J)^-1, and everything is bit-reproducible, graph-capturable and free of synchronisation."""
import numpy as np
import pytest
import torch

from test_gpu_pnp import _pose_errors, _t
from test_pnp_minimal_host import HYPOTHESES, load_robust
from test_pnp_pooled_host import POOLED_CASES, load_pooled, pooled_case

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv
from hrpe_amd.lib.core.calibrate import CameraCalibrator
from hrpe_amd.lib.utils import BPnP as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# covariance against the float64 restatement: the largest deviation over the fixture cases, relative to sqrt(cov_ii cov_jj), measured on
# an MI355X; the gate is ten times that, 1e-6 at least
COV_MEASURED = 3.13e-7
COV_GATE = max(10 * COV_MEASURED, 1e-6)


def _np(*ts):
    return [None if t is None else (t.cpu().numpy().astype(np.float64) if t.dtype.is_floating_point else t.cpu().numpy()) for t in ts]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        assert u is None or torch.equal(_bits(u), _bits(v))


def _close(P, P_ref, what, tol=1e-5):
    ang, dt = _pose_errors(np.atleast_2d(P), np.atleast_2d(P_ref))
    print(f"{what}: rotation {ang.max():.2e} rad, translation {dt.max():.2e} m")
    assert ang.max() < tol and dt.max() < tol, f"{what}: rotation {ang.max():.2e} rad, translation {dt.max():.2e} m"


def _one(x, X, K, **kw):
    """One problem: x [n,2], X [n,3] -> pnp_solve_pooled's outputs with the problem axis kept."""
    return M.pnp_solve_pooled(x.reshape(1, -1, 2), X.reshape(1, -1, 3), K, **kw)


def _fixture(c):
    x, X, K, P, Pa, mask = pooled_case(load_pooled(), c)
    return _t(x), _t(X), _t(K), P, Pa, mask


@pytest.mark.parametrize("c", list(POOLED_CASES))
def test_sequence_consensus_and_pose(c):
    x, X, K, P_ref, Pa_ref, mask = _fixture(c)
    P, inl, status, rms, cov = _np(*_one(x, X, K))
    assert np.array_equal(inl[0], mask), np.flatnonzero(inl[0] != mask)
    assert status[0, 0] & nv.PNP_NO_CONSENSUS == 0 and status[0, 0] & nv.PNP_CONVERGED and status[0, 0] & nv.PNP_FEW_POINTS == 0, status
    assert status[0, 2] == mask.sum() and status[0, 3] == 1024 and status[0, 1] > 0, status
    _close(P, P_ref, c)
    assert 0 < rms[0] < 2.0
    Pa, _, st_a, _, _ = _np(*_one(x, X, K, refine_all=True))
    _close(Pa, Pa_ref, c + " refine_all")
    assert st_a[0, 0] & nv.PNP_NO_CONSENSUS == 0 and st_a[0, 0] & nv.PNP_CONVERGED


@pytest.mark.parametrize("c", list(HYPOTHESES))
def test_agrees_with_the_robust_solver_where_both_apply(c):
    """golden_pnp_robust.npz (n = 7, 8, 17, 24), sample by sample through the pooled entry point: the same inliers, count and
    hypotheses, the pose within 1e-5 (not the same bits: the sums run in another order)."""
    g = load_robust()
    x, X, K = _t(g[f"{c}_pts2d"]), _t(g[f"{c}_pts3d"]), _t(g[f"{c}_K"])
    P0, inl0, st0, _ = _np(*M.pnp_solve_robust(x, X, K))
    full = M.pnp_solve_pooled(x, X, K)                               # the samples as the problems of one call
    P, inl, st, _, _ = _np(*full)
    assert np.array_equal(inl, inl0) and np.array_equal(st[:, 2:4], st0[:, 2:4]) and (st[:, 3] == HYPOTHESES[c]).all()
    assert np.array_equal(inl, g[f"{c}_mask"].astype(bool))
    _close(P, P0, c + " against pnp_solve_robust")
    for i in range(0, x.shape[0], 3):                                # and alone
        one = _one(x[i], X[i], K)
        _same(one, [t[i:i + 1] for t in full])


def _planted(n, seed=11):
    """n points in a box in front of a camera, exact projections of one pose; 30 % of them (none at n = 4) moved by 15 .. 60 px."""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    K = np.array([[615.0, 0, 320], [0, 615.0, 240], [0, 0, 1]])
    X = rng.uniform([-0.45, -0.45, 0.0], [0.45, 0.45, 0.9], (n, 3)).astype(np.float32).astype(np.float64)
    P = np.array([0.4, -0.3, 0.2, 0.05, -0.1, 2.0])
    from test_pnp_host import rodrigues_np
    p = (X @ rodrigues_np(P[None, :3])[0].T + P[3:]) @ K.T
    x = p[:, :2] / p[:, 2:3]
    mask = np.ones(n, bool)
    if n > 4:
        out = rng.choice(n, int(0.3 * n), replace=False)
        ang, d = rng.uniform(0, 2 * np.pi, len(out)), rng.uniform(15, 60, len(out))
        x[out] += np.stack([d * np.cos(ang), d * np.sin(ang)], 1)
        mask[out] = False
    return _t(x), _t(X), _t(K), P, mask


@pytest.mark.parametrize("n", [4, 64, 65, 255, 256, 257, 16384])
def test_sizes_where_the_layout_changes(n):
    x, X, K, P_true, mask = _planted(n)
    P, inl, status, rms, cov = _np(*_one(x, X, K))
    assert np.array_equal(inl[0], mask), (n, np.flatnonzero(inl[0] != mask)[:10])
    assert status[0, 2] == mask.sum() and status[0, 3] == min(n * (n - 1) * (n - 2) // 6, 1024) and status[0, 0] == nv.PNP_CONVERGED, status
    _close(P, P_true, f"n = {n} against the generating pose")
    assert np.isfinite(cov).all() and np.isfinite(rms).all()


def test_three_problems_in_one_call_do_not_see_each_other():
    x, X, K, _, _, mask = _fixture("f37x7")
    n = len(mask)
    valid = torch.ones(3, n, dtype=torch.bool, device=DEV)
    valid[1] = torch.tensor(mask, device=DEV)
    valid[2, :100] = False
    xs, Xs = x[None].repeat(3, 1, 1).contiguous(), X[None].repeat(3, 1, 1).contiguous()
    got = M.pnp_solve_pooled(xs, Xs, K, valid=valid)
    st = got[2].cpu().numpy()
    assert st[0, 3] == 1024 and (st[:, 0] & nv.PNP_NO_CONSENSUS == 0).all()
    assert got[1][1].sum().item() == mask.sum() and not got[1][2, :100].any() and st[2, 2] < st[0, 2] == st[1, 2]
    for b in range(3):
        _same([t[b:b + 1] for t in got], _one(x, X, K, valid=valid[b:b + 1]))


def test_unusable_points():
    x, X, K, P_ref, _, mask = _fixture("f10x7")
    ref = _one(x, X, K)
    # the planted outliers marked unusable: the same consensus, the same pose
    P, inl, status, _, _ = _np(*_one(x, X, K, valid=torch.tensor(mask[None], device=DEV)))
    assert np.array_equal(inl[0], mask) and status[0, 2] == mask.sum()
    _close(P, _np(ref[0])[0], "outliers masked against the unmasked call", tol=1e-6)
    # a NaN key-point and a NaN 3-D coordinate (two planted outliers) behave as unusable
    bad = np.flatnonzero(~mask)[[0, 3]]
    xn, Xn = x.clone(), X.clone()
    xn[bad[0], 0] = float("nan")
    Xn[bad[1], 1] = float("nan")
    got = _one(xn, Xn, K)
    v = torch.ones(1, len(mask), dtype=torch.bool, device=DEV)
    v[0, bad.tolist()] = False
    _same(got, _one(x, X, K, valid=v))
    P, inl, status, rms, cov = _np(*got)
    assert np.array_equal(inl[0], mask) and np.isfinite(P).all() and np.isfinite(rms).all() and np.isfinite(cov).all()
    _close(P, P_ref, "NaN points")
    # fewer than four usable points: both flags, finite outputs, nothing reported as an inlier that is unusable
    v = torch.zeros(1, len(mask), dtype=torch.bool, device=DEV)
    v[0, [2, 9, 30]] = True
    P, inl, status, rms, cov = _np(*_one(x, X, K, valid=v))
    assert status[0, 0] & nv.PNP_FEW_POINTS and status[0, 0] & nv.PNP_NO_CONSENSUS and status[0, 3] == 0, status
    assert np.isfinite(P).all() and np.isfinite(rms).all() and (cov == 0).all()
    assert not inl[0][~v[0].cpu().numpy()].any() and status[0, 2] == inl.sum()


def test_no_consensus():
    _, X, K, _, _, _ = _fixture("f10x7")
    rng = np.random.Generator(np.random.PCG64(21))
    x = _t(rng.random((70, 2)) * np.array([640.0, 480.0]))
    P, inl, status, rms, cov = _np(*_one(x, X, K, min_inliers=20))
    assert status[0, 0] & nv.PNP_NO_CONSENSUS and status[0, 0] & nv.PNP_FEW_POINTS == 0 and status[0, 3] == 1024, status
    assert status[0, 2] == inl.sum() < 20
    assert np.isfinite(P).all() and np.isfinite(rms).all() and np.isfinite(cov).all() and rms[0] > 3.0


# ---- covariance: s^2 (J^T J)^-1 in float64 at the returned pose over the returned inliers ------------------------------------------------
def _project_c(p, X, K):
    """Projection for a complex pose vector (complex-step derivatives): exact Rodrigues, no absolute values."""
    w, t = p[:3], p[3:]
    s = (w * w).sum()
    th = np.sqrt(s)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / s * (W @ W)
    q = (X @ R.T + t) @ K.T
    return q[:, :2] / q[:, 2:3]


def _cov_ref(P, X, x, K):
    J = np.stack([np.imag(_project_c(P.astype(complex) + 1e-30j * np.eye(6)[a], X, K)).ravel() / 1e-30 for a in range(6)], 1)
    e = (_project_c(P, X, K) - x).ravel()
    return (e @ e) / (2 * len(X) - 6) * np.linalg.inv(J.T @ J)


def test_covariance():
    worst, sig_t = 0.0, []
    for c in POOLED_CASES:
        x, X, K, _, _, mask = _fixture(c)
        P, inl, _, _, cov = _np(*_one(x, X, K))
        cov, m = cov[0], inl[0]
        xn, Xn, Kn = x.cpu().numpy().astype(np.float64), X.cpu().numpy().astype(np.float64), K.cpu().numpy().astype(np.float64)
        ref = _cov_ref(P[0], Xn[m], xn[m], Kn)
        d = np.sqrt(np.diag(ref))
        dev = (np.abs(cov - ref) / np.outer(d, d)).max()
        worst = max(worst, dev)
        print(f"{c}: covariance deviates by {dev:.2e} of sqrt(cov_ii cov_jj); sigma_t {np.sqrt(np.diag(cov))[3:]}")
        assert np.array_equal(cov, cov.T) and (np.diag(cov) > 0).all()
        sig_t.append(np.diag(cov)[3:])
    print(f"largest deviation {worst:.2e}, gate {COV_GATE:.1e}")
    assert worst <= COV_GATE, worst
    f10, f37, f150 = sig_t[:3]
    assert (f37 < f10).all() and (f150 < f37).all(), sig_t
    assert M.pnp_solve_pooled(x[None], X[None], K, want_cov=False)[4] is None


def test_bits_and_graph_capture():
    x, X, K, _, _, _ = _fixture("f9x17")
    eager = _one(x, X, K)
    _same(eager, _one(x, X, K))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _one(x, X, K)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _one(x, X, K)
    graph.replay()
    torch.cuda.synchronize()
    _same(out, eager)


# ---- CameraCalibrator ----------------------------------------------------------------------------------------------------------------------
class _Robot:
    """The caller's URDFRobot as far as the calibrator uses it: nkp and get_keypoints_only_fk, here a table looked up by q[:, 0]."""

    def __init__(self, table):
        self.table, self.nkp = table, table.shape[1]

    def get_keypoints_only_fk(self, q):
        return self.table[q[:, 0].long()]


def _frames(c):
    g = load_pooled()
    return _t(g[f"{c}_pts2d"]), _t(g[f"{c}_pts3d"]), _t(g[f"{c}_K"]), g[f"{c}_mask"].astype(bool)


def test_calibrator_collects_a_sequence_without_synchronising():
    x, X, K, mask = _frames("f37x7")
    F, k = mask.shape
    q = torch.arange(F, device=DEV, dtype=torch.float32)[:, None].repeat(1, 7)
    cal = CameraCalibrator(_Robot(X), K, capacity_frames=64, min_inliers=4, device=DEV)
    want = _one(x, X, K)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        cal.add(x[:5], q[:5])
        cal.add(x[5:6], q[5:6])
        cal.add(x[6:], q[6:])
        res = cal.solve()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(cal) == F
    _same([res.cTr[None], res.inliers.reshape(1, -1), res.status[None], res.rms[None], res.cov[None]], want)
    assert np.array_equal(res.inliers.cpu().numpy(), mask) and torch.equal(res.frame_inliers, res.inliers.sum(1))
    assert res.R.shape == (3, 3) and torch.equal(res.t, res.cTr[3:])
    assert torch.allclose(res.R, M._pose_matrix(res.cTr[None], True)[0, :, :3])
    # given 3-D points instead of joint angles; reset
    cal.reset()
    assert len(cal) == 0
    cal.add(x, None, points_3d=X)
    assert torch.equal(_bits(cal.solve().cTr), _bits(res.cTr))
    with pytest.raises(ValueError):
        CameraCalibrator(_Robot(X), K, capacity_frames=16384 // 7 + 1, device=DEV)
    CameraCalibrator(_Robot(X[:, :1].repeat(1, 8, 1)), K, capacity_frames=2048, device=DEV)      # 2048 * 8 = 16384: the largest ring


def test_calibrator_ring_keeps_the_latest_frames():
    x, X, K, _ = _frames("f37x7")
    cal = CameraCalibrator(_Robot(X), K, capacity_frames=8, min_inliers=4, device=DEV)
    cal.add(x[:4], None, points_3d=X[:4])
    cal.add(x[4:11], None, points_3d=X[4:11])
    assert len(cal) == 8
    res = cal.solve()
    _same([res.cTr[None], res.inliers.reshape(1, -1), res.status[None], res.rms[None], res.cov[None]], _one(x[3:11], X[3:11], K))
    cal.add(x[11:31], None, points_3d=X[11:31])                      # more frames in one call than the ring holds
    assert torch.equal(_bits(cal.solve().cTr), _bits(_one(x[23:31], X[23:31], K)[0][0]))


def test_calibrator_add_detection_drops_weak_peaks():
    x, X, K, _ = _frames("f10x7")
    F, k = x.shape[:2]
    rng = np.random.Generator(np.random.PCG64(4))
    strong = torch.tensor(rng.random((F, k)) > 0.2, device=DEV)
    peak = torch.where(strong, torch.tensor(0.9, device=DEV), torch.tensor(0.1, device=DEV))
    ms = torch.stack([torch.zeros_like(peak), 1.0 / peak], -1)
    cal = CameraCalibrator(_Robot(X), K, capacity_frames=16, min_inliers=4, device=DEV)
    cal.add_detection(x * 0.5, ms, torch.arange(F, device=DEV, dtype=torch.float32)[:, None], scale=0.5, min_peak=0.3)
    assert torch.equal(cal.frames()[2], strong) and torch.equal(cal.frames()[0], x)
    res = cal.solve()
    want = _one(x, X, K, valid=strong.reshape(1, -1))
    assert torch.equal(_bits(res.cTr), _bits(want[0][0])) and torch.equal(res.inliers.reshape(1, -1), want[1])
    assert not res.inliers[~strong].any()


def test_ctrnet_inference_sequence():
    from hrpe_amd.lib.models.ctrnet.mask_inference import seg_mask_inference
    torch.manual_seed(5)
    net = seg_mask_inference((60.0, 60.0, 48.0, 32.0), "azure", image_hw=(128, 192), allow_random_init=True).to(DEV).net
    img = torch.randn(2, 3, 64, 96, device=DEV)
    pts = (torch.rand(2, 7, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV) + torch.tensor([0.0, 0.0, 1.5], device=DEV)
    with torch.no_grad():
        p2d, fg = net.inference_batch_images_seg_kp(img)
        cTr, p2, fg2 = net.inference_sequence(img, None, points_3d=pts)
    want = M.pnp_solve_pooled(p2d.reshape(1, 14, 2), pts.reshape(1, 14, 3), net.K, want_cov=False)
    assert cTr.shape == (1, 6) and torch.equal(_bits(cTr), _bits(want[0])) and torch.equal(p2, p2d) and torch.equal(fg2, fg)
    assert net.last_inliers.shape == (2, 7) and torch.equal(net.last_inliers, want[1].reshape(2, 7))
