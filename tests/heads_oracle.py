"""Oracle of the pose-head kernels (csrc/heads.hip), restated from include/hrp.h and the kernel comments in plain torch on the CPU.

Every function takes `dt`: torch.float64 is the oracle, torch.float32 the restatement the arithmetic tests measure their noise floor
with (same formulas, torch's own evaluation order - nothing of the kernels' loops is copied).  Gradients come from autograd on these
forwards (`vjp`).  Proved on the CPU against oracle/heads.py, oracle/fk.py and the reference's fixtures in test_heads_oracle_host.py.

In fp32 the soft-argmax evaluates its exponential the way the device does: HIP's __expf is exp2 of the fp32 product x * log2(e)
(__clang_hip_math.h), and the rounding of that product - up to |x| 2^-24 in the exponent - dominates the error of a weight."""
import numpy as np
import torch

from oracle.fk import rot6d_to_rotmat, rotmat_to_quat, rotmat_to_rot6d

F64, F32 = torch.float64, torch.float32
LOG2E = float(np.float32(1.4426950408889634))       # 0x1.715476p+0
EPS24 = 2.0 ** -24


def f32(v):
    """A host float as the kernel sees it (float arguments of the C ABI)."""
    return float(np.float32(v))


def dev_exp(x):
    return torch.exp(x) if x.dtype == F64 else torch.exp2(x * torch.tensor(LOG2E, dtype=x.dtype))


def vjp(fn, inputs, cots, dt=F64):
    """Gradients of sum_k <out_k, cot_k> with respect to `inputs` (cot None: that output carries no gradient); fn maps the leaves
    (in dt) to a tuple of outputs."""
    leaves = [x.detach().to(dt).clone().requires_grad_(True) for x in inputs]
    outs = fn(*leaves)
    terms = [(o * c.to(dt)).sum() for o, c in zip(outs, cots) if c is not None and o is not None]
    if not terms:
        return [torch.zeros_like(x) for x in leaves]
    g = torch.autograd.grad(sum(terms), leaves, allow_unused=True)
    return [torch.zeros_like(x) if v is None else v for x, v in zip(leaves, g)]


# ---- soft-argmax ----------------------------------------------------------------------------------------------------------------
def softargmax3d(logits, J, D, root=0, fix_root=0, dt=F64):
    """logits [B, H, W, J * D] (channel j * D + d: the channel index within a joint is the depth bin) -> uvd [B, J, 3] in
    [-0.5, 0.5), ms [B, J, 2] = (max, sum of exp(x - max))."""
    B, H, W, _ = logits.shape
    x = logits.to(dt).reshape(B, H * W, J, D).permute(0, 2, 1, 3)          # [B, J, HW, D]
    m = x.amax((2, 3)).detach()
    e = dev_exp(x - m[:, :, None, None])
    s = e.sum((2, 3))
    p = torch.arange(H * W)
    xs, ys, ds = (p % W).to(dt), (p // W).to(dt), torch.arange(D).to(dt)
    ep = e.sum(3)
    u = (ep * xs).sum(2) / s / W - 0.5
    v = (ep * ys).sum(2) / s / H - 0.5
    d = (e.sum(2) * ds).sum(2) / s / D - 0.5
    if fix_root:
        keep = torch.ones(J, dtype=dt)
        keep[root] = 0
        d = d * keep
    return torch.stack((u, v, d), 2), torch.stack((m, s), 2)


def softargmax_flat(logits, dt=F64):
    """logits [B, HW, J] -> coord [B, J] = E[flat index] / HW, ms [B, J, 2]."""
    x = logits.to(dt)
    HW = x.shape[1]
    m = x.amax(1).detach()
    e = dev_exp(x - m[:, None, :])
    s = e.sum(1)
    coord = (e * torch.arange(HW).to(dt)[None, :, None]).sum(1) / s / HW
    return coord, torch.stack((m, s), 2)


# ---- camera geometry ------------------------------------------------------------------------------------------------------------
def inv_intrinsics(K, dt=F64):
    """(1 / fx, -cx / fx, 1 / fy, -cy / fy): an fp64 divide rounded to fp32 (oracle/heads.inv_intrinsics), then in dt."""
    fx, fy, cx, cy = K[:, 0, 0].double(), K[:, 1, 1].double(), K[:, 0, 2].double(), K[:, 1, 2].double()
    return [t.float().to(dt) for t in (1.0 / fx, -cx / fx, 1.0 / fy, -cy / fy)]


def pose_geometry(gamma, kval, uvd, K, root, S, DF, dt=F64):
    """gamma [B], kval [B], uvd [B, J, 3], K [B, 3, 3] -> depth [B], xyz [B, J, 3], root_uv [B, 2], trans [B, 3]:
    depth = gamma k / 1000; xyz_j = K^-1 (U, V, 1) (d_j DF + depth) with (U, V) = (uv_j + 0.5) S; root_uv = (U, V) of the root;
    trans = K^-1 (root_uv depth, depth)."""
    a, b, c, d = inv_intrinsics(K, dt)
    S, DF = f32(S), f32(DF)
    gamma, kval, uvd = gamma.to(dt), kval.to(dt), uvd.to(dt)
    z = gamma * kval / 1000.0
    U, V = (uvd[..., 0] + 0.5) * S, (uvd[..., 1] + 0.5) * S
    za = uvd[..., 2] * DF + z[:, None]
    xyz = torch.stack(((a[:, None] * U + b[:, None]) * za, (c[:, None] * V + d[:, None]) * za, za), 2)
    ru, rv = U[:, root], V[:, root]
    trans = torch.stack((a * (ru * z) + b * z, c * (rv * z) + d * z, z), 1)
    return z, xyz, torch.stack((ru, rv), 1), trans


# ---- kinematics -----------------------------------------------------------------------------------------------------------------
def _rigid(R, t):
    B = R.shape[0]
    T = torch.zeros(B, 4, 4, dtype=R.dtype)
    T[:, 3, 3] = 1
    return torch.cat((torch.cat((R, t[:, :, None]), 2), T[:, 3:, :]), 1)


def _rigid_inv(T):
    Rt = T[:, :3, :3].transpose(1, 2)
    return _rigid(Rt, -(Rt @ T[:, :3, 3:])[:, :, 0])


def _joint(chain, j, q, dt):
    """origin_j motion_j(mimic_mul_j q[cfg_j] + mimic_off_j) [B, 4, 4]."""
    B = q.shape[0]
    O = torch.eye(4, dtype=dt)
    O[:3, :] = torch.tensor([float(v) for v in chain.origin[j]], dtype=dt).view(3, 4)
    O = O.expand(B, 4, 4)
    typ, cfg = int(chain.type[j]), int(chain.cfg[j])
    if typ == 0 or cfg < 0:
        return O
    qv = float(chain.mimic_mul[j]) * q[:, cfg] + float(chain.mimic_off[j])
    a = torch.tensor([float(v) for v in chain.axis[j]], dtype=dt)
    eye = torch.eye(3, dtype=dt)
    if typ == 1:
        skew = torch.zeros(3, 3, dtype=dt)
        skew[0, 1], skew[0, 2], skew[1, 0], skew[1, 2], skew[2, 0], skew[2, 1] = -a[2], a[1], a[2], -a[0], -a[1], a[0]
        s, c = torch.sin(qv)[:, None, None], torch.cos(qv)[:, None, None]
        M = _rigid(c * eye + (1 - c) * torch.outer(a, a) + s * skew, torch.zeros(B, 3, dtype=dt))
    else:
        M = _rigid(eye.expand(B, 3, 3), qv[:, None] * a)
    return O @ M


def frames(chain, q, dt=F64):
    """-> f(j): pose [B, 4, 4] of joint j's child frame in the base (j = -1: the base itself), T_j = T_parent(j) origin_j motion_j."""
    q = q.to(dt)
    B = q.shape[0]
    cache = {-1: torch.eye(4, dtype=dt).expand(B, 4, 4)}

    def f(j):
        if j not in cache:
            cache[j] = f(int(chain.parent[j])) @ _joint(chain, j, q, dt)
        return cache[j]
    return f


def base_to_cam(rot, trans, dt=F64):
    rot, trans = rot.to(dt), trans.to(dt)
    if rot.shape[1] == 6:
        return _rigid(rot6d_to_rotmat(rot), trans)
    n = rot / (torch.sqrt((rot * rot).sum(1, keepdim=True)) + 1e-9)
    w, x, y, z = n[:, 0], n[:, 1], n[:, 2], n[:, 3]
    R = torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                     2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                     2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], 1).view(-1, 3, 3)
    return _rigid(R, trans)


def project(K, pts, dt=F64):
    """uv = (K p)[:2] / (K p)[2] with all nine entries of K [B, 3, 3]; pts [B, P, 3]."""
    h = torch.einsum("bij,bkj->bki", K.to(dt), pts.to(dt))
    return h[..., :2] / h[..., 2:3]


def fk(chain, q, rot, trans, K=None, root=0, dt=F64):
    """An interpreter of the nv.FkChain fields.  -> xyz [B, nkp, 3] (camera frame, re-rooted at key point `root` when root > 0),
    uv [B, nkp, 2] (None without K), root_rot [B, rot_dim]: (B2C T_root).R as its first two rows or its quaternion."""
    f = frames(chain, q, dt)
    B2C = base_to_cam(rot, trans, dt)
    M = B2C
    if root > 0:
        M = M @ _rigid_inv(f(int(chain.kp_frame[root])))
    pts = []
    for k in range(int(chain.nkp)):
        off = torch.tensor([float(v) for v in chain.kp_offset[k]] + [1.0], dtype=dt)
        pts.append(((M @ f(int(chain.kp_frame[k]))) @ off)[:, :3])
    xyz = torch.stack(pts, 1)
    P = B2C @ f(int(chain.kp_frame[root])) if root > 0 else B2C
    rr = rotmat_to_rot6d(P[:, :3, :3]) if rot.shape[1] == 6 else rotmat_to_quat(P[:, :3, :3])
    return xyz, (project(K, xyz, dt) if K is not None else None), rr


def rot6d_compose(a, b, dt=F64):
    return rotmat_to_rot6d(rot6d_to_rotmat(a.to(dt)) @ rot6d_to_rotmat(b.to(dt)))


def mesh_pose(chain, q, rot6d, trans, root_kp, verts, vert_link, K=None, dt=F64):
    """xyz[b, v] = s_b M_b T_link(v) verts[v], M = B2C (root_kp < 0) or B2C T_root^-1, s_b = -1 (a mirror through the origin, a
    constant for autograd) when M_b's translation has negative z.  -> xyz [B, V, 3], uv or None, s [B]."""
    f = frames(chain, q, dt)
    M = base_to_cam(rot6d, trans, dt)
    if root_kp >= 0:
        M = M @ _rigid_inv(f(int(chain.kp_frame[root_kp])))
    s = torch.where(M[:, 2, 3] < 0, -1.0, 1.0).to(dt).detach()
    TL = torch.stack([f(int(chain.kp_frame[k])) for k in range(int(chain.nkp))], 1)          # [B, L, 4, 4]
    vh = torch.cat((verts.to(dt), torch.ones(verts.shape[0], 1, dtype=dt)), 1)
    posed = torch.einsum("bvij,vj->bvi", (M[:, None] @ TL)[:, vert_link.long()], vh)[..., :3] * s[:, None, None]
    return posed, (project(K, posed, dt) if K is not None else None), s


# ---- losses ---------------------------------------------------------------------------------------------------------------------
def l1_loss(pred, gt, scale, dt=F64):
    return (pred.to(dt) * f32(scale) - gt.to(dt)).abs().mean()


PRED = ("pose", "rot", "trans", "root_uv", "depth", "xyz_int", "xyz_fk")
# out[k] of hrp_pose_loss and the index into hrp_pose_loss_desc.weights (pose, rot, uv, depth, trans, kp2d, kp3d, kp2d_int, kp3d_int,
# align_3d) that multiplies it
TERMS = ("loss_joint", "loss_rot", "loss_uv", "loss_depth", "loss_trans", "loss_error3d", "loss_error2d", "loss_error2d_int",
         "loss_error3d_int", "loss_error3d_align")
TERM_WEIGHT = (0, 1, 2, 3, 4, 6, 5, 7, 8, 9)


def pose_loss(pred, gt, K, weights, root, S, rot_dim=6, dt=F64):
    """oracle/heads.full_loss with the ten weights of hrp_pose_loss_desc.  pred: the seven tensors of PRED (pose [B, P], rot
    [B, rot_dim], trans [B, 3], root_uv [B, 2], depth [B, 1], xyz_int, xyz_fk [B, J, 3]); gt: pose, root_rot, root_trans, root_uv,
    kp3d, kp2d, mask.  -> out [11]: the terms in TERMS order, then the weighted total."""
    pose, rot, trans, root_uv, depth, xyz_int, xyz_fk = [t.to(dt) for t in pred]
    g = {k: v.to(dt) for k, v in gt.items()}
    S = f32(S)
    assert rot.shape[1] == rot_dim
    m = g["mask"]
    nrm = lambda v: torch.norm(v, dim=-1)          # noqa: E731
    t = [((pose - g["pose"]) ** 2).mean(), ((rot - g["root_rot"]) ** 2).mean(),
         (nrm((root_uv - g["root_uv"]) / S) * m[:, root]).sum() / (m[:, root] != 0).sum(),
         (depth - g["root_trans"][:, 2:3]).abs().mean()]
    e = nrm(trans - g["root_trans"])
    t.append((e * torch.exp(-20.0 * e).detach()).mean() if e.mean() > 0.5 else e.mean())
    gt2d = g["kp2d"] / S
    nv = (m != 0).sum()
    t += [nrm(xyz_fk - g["kp3d"]).mean(), (nrm(project(K, xyz_fk, dt) / S - gt2d) * m).sum() / nv,
          (nrm(project(K, xyz_int, dt) / S - gt2d) * m).sum() / nv, nrm(xyz_int - g["kp3d"]).mean(), nrm(xyz_fk - xyz_int).mean()]
    total = sum(f32(weights[w]) * v for w, v in zip(TERM_WEIGHT, t))
    return torch.stack(t + [total])


def pose_loss_inputs(seed, B, damped, J=7, P=8, R=6, root=3, zero_row=None):
    """The recipe of test_fused_pose_loss_matches_tensor_expressions: random predictions around a ground truth 1.2 m in front of
    the camera, mask entries zero with probability 0.2 and mask[0, root] = 0, xyz_int[1, 2] exactly on target, translation errors
    on either side of the damping threshold.  -> pred (the seven tensors of PRED), gt, K, uvd (full_loss's sixth prediction)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 300.0 + 200.0 * torch.rand(B, generator=g)
    K[:, 0, 2] = K[:, 1, 2] = 128.0
    K[:, 2, 2] = 1.0
    kp3d = r(B, J, 3) * 0.3 + torch.tensor([0.0, 0.0, 1.2])
    gt = dict(pose=r(B, P), root_rot=r(B, R), root_trans=kp3d[:, root].clone(), root_uv=128 + 40 * r(B, 2), kp3d=kp3d,
              kp2d=128 + 60 * r(B, J, 2), mask=(torch.rand(B, J, generator=g) > 0.2).float())
    if B > 1:                                   # (with one sample the root term would be 0 / 0)
        gt["mask"][0, root] = 0.0
    else:
        gt["mask"][0, root] = 1.0
    if zero_row is not None:
        gt["mask"][zero_row] = 0.0
    pred =[r(B, P), r(B, R), kp3d[:, root] + (2.0 if damped else 0.05) * r(B, 3), 128 + 40 * r(B, 2), 1.2 + 0.2 * r(B, 1),
            r(B, J, 3), kp3d + 0.1 * r(B, J, 3), kp3d + 0.1 * r(B, J, 3)]
    pred[6][min(1, B - 1), 2] = kp3d[min(1, B - 1), 2]       # exactly on target: ||.|| = 0 -> gradient 0
    return pred[:5] + pred[6:], gt, K, pred[5]


def floor_of(v32, v64):
    """The fp32 noise floor of a tensor: max |fp32 - fp64| relative to max |fp64|, never below one fp32 rounding."""
    sc = float(v64.abs().max())
    return max(float((v32.to(F64) - v64).abs().max()) / sc, EPS24) if sc > 0 else EPS24
