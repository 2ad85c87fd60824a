"""Back-propagatable PnP with the reference's names (lib/utils/BPnP.py), on the GPU.

``BPnP`` (shared pts3d [n,3]), ``BPnP_m3d`` (pts3d [B,n,3]) and ``BPnP_fast`` take ``(pts2d [B,n,2], pts3d, K [3,3], ini_pose=None)``
and return P_6d [B,6] (angle-axis with |w| <= pi, then translation) in fp32 on pts2d's device.  K may also be [B,3,3].

Forward (csrc/pnp.hip hrp_pnp_solve): one launch for the batch.  EPnP gives the start (the reference's cv2.solvePnP SOLVEPNP_EPNP,
BPnP.py:36, 140), or ``ini_pose`` does (:142-145); Levenberg-Marquardt on the reprojection error then refines it (SOLVEPNP_ITERATIVE
with useExtrinsicGuess, :41, 146).  ``BPnP_fast`` starts from the same EPnP solution.
Robust forward (hrp_pnp_solve_robust, ``pnp_solve_robust`` / ``BPnP_robust``): the reference's RANSAC start (cv2.solvePnPRansac with
reprojectionError = 3, :267) as one launch: consensus over P3P hypotheses, then the same LM on the inliers, refitted while the inlier set
changes; ``refine_all`` adds the LM over all points that BPnP_fast runs from there (:268-271).  It differs from cv2 in two ways, so
parity is by objective, not by bits: the minimal sets are enumerated (every triple, or a fixed hash-drawn list of ``max_hypotheses``
triples where there are more), not sampled until a confidence is reached, and each is solved by P3P, not by five-point EPnP.  The
result is deterministic.  Its backward is the gradient below restricted to the inliers (hrp_pnp_bwd_masked), or BPnP_fast's over all
points with ``refine_all``.
Pooled forward (hrp_pnp_solve_pooled, ``pnp_solve_pooled``): the robust forward's semantics for up to 16384 points per problem, three
launches (compact, score on a grid, fit in one workgroup), with the covariance of the pose: one camera pose from all the key-points of
a sequence (lib/core/calibrate.py).  No backward.
Backward (hrp_pnp_bwd): the reference's formula, -g^T J_fy^-1 J_f(x, z, K) (:50-111, 154-236), with the derivatives of get_coefs'
coefficients kept, or dropped for ``BPnP_fast`` (:280-341).  The forward's rotation is the exact Rodrigues formula (cv2's); the
backward differentiates the rotation the reference's backward uses (kornia's: axis = w / (theta + 1e-6), first-order below
theta^2 = 1e-6), whose ~1e-6 / theta relative difference the 6 x 6 inverse amplifies to ~2e-4 of the gradients at theta ~ 0.14.
A singular J_fy gives NaN gradients for that sample (the reference raises in torch.inverse)."""
import ctypes

import torch

from hrpe_amd import _native as nv
from hrpe_amd.lib.utils.geometries import angle_axis_to_rotation_matrix
from hrpe_amd.lib.utils.transforms import point_projection_from_3d_tensor


def _check(pts2d, pts3d, K, ini_pose, shared):
    for name, t in (("pts2d", pts2d), ("pts3d", pts3d), ("K", K)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError(f"BPnP: {name} must be a CUDA tensor (there is no CPU path)")
    if pts2d.dim() != 3 or pts2d.shape[2] != 2:
        raise ValueError(f"BPnP: pts2d must be [B, n, 2], got {tuple(pts2d.shape)}")
    B, n = pts2d.shape[0], pts2d.shape[1]
    if n < 4 or n > 64:
        raise ValueError(f"BPnP: {n} points; the solver needs 4 <= n <= 64")
    want = (n, 3) if shared else (B, n, 3)
    if tuple(pts3d.shape) != want:
        raise ValueError(f"BPnP: pts3d must be {list(want)}, got {list(pts3d.shape)}")
    if tuple(K.shape) not in ((3, 3), (B, 3, 3)):
        raise ValueError(f"BPnP: K must be [3, 3] or [B, 3, 3], got {list(K.shape)}")
    if ini_pose is not None and tuple(ini_pose.shape) != (B, 6):
        raise ValueError(f"BPnP: ini_pose must be [B, 6], got {list(ini_pose.shape)}")


def _f32(t):
    return t.detach().contiguous().float()


def pnp_solve(pts2d, pts3d, K, ini_pose=None, shared=None):
    """P_6d [B,6], status [B,2] int32 (converged, iterations), rms [B] (reprojection error, px).  No autograd."""
    if shared is None:
        shared = pts3d.dim() == 2
    _check(pts2d, pts3d, K, ini_pose, shared)
    B, n = pts2d.shape[0], pts2d.shape[1]
    dev = pts2d.device
    x, z, k = _f32(pts2d), _f32(pts3d), _f32(K)
    ini = _f32(ini_pose.to(dev)) if ini_pose is not None else None
    P = torch.empty(B, 6, device=dev)
    status = torch.empty(B, 2, dtype=torch.int32, device=dev)
    rms = torch.empty(B, device=dev)
    nv.call("hrp_pnp_solve", x.data_ptr(), z.data_ptr(), 0 if shared else 3 * n, k.data_ptr(), 0 if k.dim() == 2 else 9,
            ini.data_ptr() if ini is not None else None, B, n, P.data_ptr(), status.data_ptr(), rms.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    return P, status, rms


def pnp_backward(pts2d, pts3d, K, P_6d, grad_output, fast=False, shared=None):
    """(grad_x [B,n,2], grad_z [n,3] or [B,n,3], grad_K [3,3] or [B,3,3], status [B] int32: 1 = singular J_fy)."""
    if shared is None:
        shared = pts3d.dim() == 2
    B, n = pts2d.shape[0], pts2d.shape[1]
    dev = pts2d.device
    x, z, k, P, g = _f32(pts2d), _f32(pts3d), _f32(K), _f32(P_6d), _f32(grad_output)
    k_shared = k.dim() == 2
    gx = torch.empty(B, n, 2, device=dev)
    gz = torch.empty(B, n, 3, device=dev)
    gK = torch.empty(B, 3, 3, device=dev)
    gz_sum = torch.empty(n, 3, device=dev) if shared else None
    gK_sum = torch.empty(3, 3, device=dev) if k_shared else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nv.call("hrp_pnp_bwd", x.data_ptr(), z.data_ptr(), 0 if shared else 3 * n, k.data_ptr(), 0 if k_shared else 9, P.data_ptr(),
            g.data_ptr(), B, n, int(fast), gx.data_ptr(), gz.data_ptr(), gK.data_ptr(),
            gz_sum.data_ptr() if shared else None, gK_sum.data_ptr() if k_shared else None, status.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    return gx, (gz_sum if shared else gz), (gK_sum if k_shared else gK), status


def pnp_solve_robust(pts2d, pts3d, K, reproj_error=3.0, valid=None, min_inliers=4, max_hypotheses=1024, seed=0, refine_all=False):
    """Consensus over P3P hypotheses, then LM on the inliers (and over all usable points with ``refine_all``): P_6d [B,6], inliers
    [B,n] bool (the points within ``reproj_error`` px of P_6d), status [B,4] int32 (HRP_PNP_* flags, LM trials, inlier count,
    hypotheses scored) and rms [B] over the points of the last fit.  ``valid`` [B,n] marks the usable points; a point with a
    non-finite coordinate is unusable too.  Below ``min_inliers`` the flag _native.PNP_NO_CONSENSUS is set and P_6d is ``pnp_solve``'s
    over the usable points.  No autograd, no synchronisation: graph-capturable."""
    shared = pts3d.dim() == 2
    _check(pts2d, pts3d, K, None, shared)
    B, n = pts2d.shape[0], pts2d.shape[1]
    dev = pts2d.device
    x, z, k = _f32(pts2d), _f32(pts3d), _f32(K)
    v = None
    if valid is not None:
        if tuple(valid.shape) != (B, n):
            raise ValueError(f"BPnP: valid must be [{B}, {n}], got {list(valid.shape)}")
        v = (valid.to(dev) != 0).to(torch.uint8).contiguous()
    P = torch.empty(B, 6, device=dev)
    inl = torch.empty(B, n, dtype=torch.uint8, device=dev)
    status = torch.empty(B, 4, dtype=torch.int32, device=dev)
    rms = torch.empty(B, device=dev)
    nv.call("hrp_pnp_solve_robust", x.data_ptr(), z.data_ptr(), 0 if shared else 3 * n, k.data_ptr(), 0 if k.dim() == 2 else 9,
            v.data_ptr() if v is not None else None, B, n, float(reproj_error), int(min_inliers), int(max_hypotheses), int(seed),
            int(bool(refine_all)), P.data_ptr(), inl.data_ptr(), status.data_ptr(), rms.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    return P, inl.bool(), status, rms


def _check_pooled(pts2d, pts3d, K, valid):
    for name, t in (("pts2d", pts2d), ("pts3d", pts3d), ("K", K)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError(f"pnp_solve_pooled: {name} must be a CUDA tensor (there is no CPU path)")
    if pts2d.dim() != 3 or pts2d.shape[2] != 2:
        raise ValueError(f"pnp_solve_pooled: pts2d must be [B, n, 2], got {tuple(pts2d.shape)}")
    B, n = pts2d.shape[0], pts2d.shape[1]
    if n < 4 or n > nv.PNP_POOLED_MAX_N:
        raise ValueError(f"pnp_solve_pooled: {n} points; the solver needs 4 <= n <= {nv.PNP_POOLED_MAX_N}")
    if tuple(pts3d.shape) != (B, n, 3):
        raise ValueError(f"pnp_solve_pooled: pts3d must be [{B}, {n}, 3], got {list(pts3d.shape)}")
    if tuple(K.shape) not in ((3, 3), (B, 3, 3)):
        raise ValueError(f"pnp_solve_pooled: K must be [3, 3] or [B, 3, 3], got {list(K.shape)}")
    if valid is not None and tuple(valid.shape) != (B, n):
        raise ValueError(f"pnp_solve_pooled: valid must be [{B}, {n}], got {list(valid.shape)}")


def pnp_solve_pooled(pts2d, pts3d, K, reproj_error=3.0, valid=None, min_inliers=4, max_hypotheses=1024, seed=0, refine_all=False,
                     want_cov=True):
    """``pnp_solve_robust``'s consensus and refit for up to 16384 points per problem (hrp_pnp_solve_pooled, csrc/pnp_pooled.hip): the
    solver behind one camera pose from a whole sequence.  pts2d [B,n,2], pts3d [B,n,3], K [3,3] or [B,3,3] -> P_6d [B,6], inliers
    [B,n] bool, status [B,4] int32 (HRP_PNP_* flags, LM trials, inlier count, hypotheses scored), rms [B] over the points of the last
    fit, and cov [B,6,6] = s^2 (J^T J)^-1 in (angle-axis, t) at P_6d over those points (None without ``want_cov``).  Below
    ``min_inliers`` the flag _native.PNP_NO_CONSENSUS is set and P_6d is the LM over all usable points from the best hypothesis.
    The workspace is a tensor this call owns.  No autograd, no synchronisation: graph-capturable."""
    _check_pooled(pts2d, pts3d, K, valid)
    B, n = pts2d.shape[0], pts2d.shape[1]
    dev = pts2d.device
    x, z, k = _f32(pts2d), _f32(pts3d), _f32(K)
    v = (valid.to(dev) != 0).to(torch.uint8).contiguous() if valid is not None else None
    need = ctypes.c_size_t(0)
    nv.call("hrp_pnp_pooled_workspace_bytes", B, n, int(max_hypotheses), ctypes.byref(need))
    ws = torch.empty((need.value + 15) // 16 * 2, dtype=torch.float64, device=dev)
    P = torch.empty(B, 6, device=dev)
    inl = torch.empty(B, n, dtype=torch.uint8, device=dev)
    status = torch.empty(B, 4, dtype=torch.int32, device=dev)
    rms = torch.empty(B, device=dev)
    cov = torch.empty(B, 6, 6, device=dev) if want_cov else None
    nv.call("hrp_pnp_solve_pooled", x.data_ptr(), z.data_ptr(), k.data_ptr(), 0 if k.dim() == 2 else 9,
            v.data_ptr() if v is not None else None, B, n, float(reproj_error), int(min_inliers), int(max_hypotheses), int(seed),
            int(bool(refine_all)), ws.data_ptr(), ws.numel() * 8, P.data_ptr(), inl.data_ptr(), status.data_ptr(), rms.data_ptr(),
            cov.data_ptr() if want_cov else None, torch.cuda.current_stream(dev).cuda_stream)
    return P, inl.bool(), status, rms, cov


def pnp_backward_masked(pts2d, pts3d, K, P_6d, grad_output, mask, fast=False, shared=None):
    """``pnp_backward`` over the points of ``mask`` [B,n]: the others contribute nothing and get zero grad_x / grad_z rows."""
    if shared is None:
        shared = pts3d.dim() == 2
    B, n = pts2d.shape[0], pts2d.shape[1]
    dev = pts2d.device
    x, z, k, P, g = _f32(pts2d), _f32(pts3d), _f32(K), _f32(P_6d), _f32(grad_output)
    m = (mask.to(dev) != 0).to(torch.uint8).contiguous()
    k_shared = k.dim() == 2
    gx = torch.empty(B, n, 2, device=dev)
    gz = torch.empty(B, n, 3, device=dev)
    gK = torch.empty(B, 3, 3, device=dev)
    gz_sum = torch.empty(n, 3, device=dev) if shared else None
    gK_sum = torch.empty(3, 3, device=dev) if k_shared else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nv.call("hrp_pnp_bwd_masked", x.data_ptr(), z.data_ptr(), 0 if shared else 3 * n, k.data_ptr(), 0 if k_shared else 9, P.data_ptr(),
            g.data_ptr(), m.data_ptr(), B, n, int(fast), gx.data_ptr(), gz.data_ptr(), gK.data_ptr(),
            gz_sum.data_ptr() if shared else None, gK_sum.data_ptr() if k_shared else None, status.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    return gx, (gz_sum if shared else gz), (gK_sum if k_shared else gK), status


def _forward(ctx, shared, pts2d, pts3d, K, ini_pose):
    _check(pts2d, pts3d, K, ini_pose, shared)
    P_6d, _, _ = pnp_solve(pts2d, pts3d, K, ini_pose, shared=shared)
    ctx.save_for_backward(pts2d, P_6d, pts3d, K)
    return P_6d


def _backward(ctx, shared, fast, grad_output):
    pts2d, P_6d, pts3d, K = ctx.saved_tensors
    gx, gz, gK, _ = pnp_backward(pts2d, pts3d, K, P_6d, grad_output, fast=fast, shared=shared)
    return gx.to(pts2d.dtype), gz.to(pts3d.dtype), gK.to(K.dtype), None


class BPnP(torch.autograd.Function):
    """pts3d [n, 3] shared by every sample of the batch (BPnP.py:9-111)."""

    @staticmethod
    def forward(ctx, pts2d, pts3d, K, ini_pose=None):
        return _forward(ctx, True, pts2d, pts3d, K, ini_pose)

    @staticmethod
    def backward(ctx, grad_output):
        return _backward(ctx, True, False, grad_output)


class BPnP_m3d(torch.autograd.Function):
    """pts3d [B, n, 3]: sample i's 2-D points correspond to sample i's 3-D points (BPnP.py:114-236)."""

    @staticmethod
    def forward(ctx, pts2d, pts3d, K, ini_pose=None):
        return _forward(ctx, False, pts2d, pts3d, K, ini_pose)

    @staticmethod
    def backward(ctx, grad_output):
        return _backward(ctx, False, False, grad_output)


class BPnP_fast(torch.autograd.Function):
    """BPnP with the coefficient derivatives dropped from the backward (BPnP.py:239-341); EPnP start (the RANSAC start: BPnP_robust)."""

    @staticmethod
    def forward(ctx, pts2d, pts3d, K, ini_pose=None):
        return _forward(ctx, True, pts2d, pts3d, K, ini_pose)

    @staticmethod
    def backward(ctx, grad_output):
        return _backward(ctx, True, True, grad_output)


class BPnP_robust(torch.autograd.Function):
    """``pnp_solve_robust`` with a backward; pts3d [n, 3] shared or [B, n, 3].  ``BPnP_robust.apply(...)`` returns (P_6d, inliers [B, n]
    bool, not differentiable).  refine_all=False: the implicit-function gradient at the optimum over the inliers (outliers get zero
    rows).  refine_all=True: BPnP_fast's backward over all points (BPnP.py:280-341)."""

    @staticmethod
    def forward(ctx, pts2d, pts3d, K, reproj_error=3.0, refine_all=False):
        P_6d, inliers, _, _ = pnp_solve_robust(pts2d, pts3d, K, reproj_error=reproj_error, refine_all=refine_all)
        ctx.save_for_backward(pts2d, P_6d, pts3d, K, inliers)
        ctx.refine_all = bool(refine_all)
        ctx.mark_non_differentiable(inliers)
        return P_6d, inliers

    @staticmethod
    def backward(ctx, grad_output, _grad_inliers=None):
        pts2d, P_6d, pts3d, K, inliers = ctx.saved_tensors
        if ctx.refine_all:
            gx, gz, gK, _ = pnp_backward(pts2d, pts3d, K, P_6d, grad_output, fast=True)
        else:
            gx, gz, gK, _ = pnp_backward_masked(pts2d, pts3d, K, P_6d, grad_output, inliers)
        return gx.to(pts2d.dtype), gz.to(pts3d.dtype), gK.to(K.dtype), None, None


def batch_project(P, pts3d, K, angle_axis=True):
    """P [B,6] angle-axis + t (or [B,3,4] with angle_axis=False), pts3d [n,3], K [3,3] -> [B,n,2] (BPnP.py:359-377)."""
    PM = _pose_matrix(P, angle_axis)
    bs = PM.shape[0]
    cam = batch_transform_3d(PM, pts3d, angle_axis=False)
    return point_projection_from_3d_tensor(K.expand(bs, 3, 3).contiguous(), cam)


def batch_transform_3d(P, pts3d, angle_axis=True):
    """P [B,6] (or [B,3,4]), pts3d [n,3] -> camera-frame points [B,n,3] (BPnP.py:379-392)."""
    PM = _pose_matrix(P, angle_axis)
    n = pts3d.shape[0]
    pts3d_h = torch.cat((pts3d, torch.ones(n, 1, device=pts3d.device, dtype=pts3d.dtype)), dim=-1)
    return pts3d_h.matmul(PM.transpose(-2, -1))


def _pose_matrix(P, angle_axis):
    if not angle_axis:
        return P
    bs = P.shape[0]
    R = angle_axis_to_rotation_matrix(P[:, 0:3].reshape(bs, 3))
    return torch.cat((R[:, 0:3, 0:3], P[:, 3:6].reshape(bs, 3, 1)), dim=-1)
