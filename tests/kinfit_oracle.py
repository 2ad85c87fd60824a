"""The float64 numpy statement of hrp_kin_solve (include/hrp.h), written from the header's semantics and shared by
tests/golden/gen_golden_kinfit.py, tests/test_kinfit_host.py and tests/test_gpu_kinfit.py: FK from the chain tables, the cost and its
residual rows, a complex-step Jacobian, the kernel's LM schedule restated, and the packing of a case for tests/kinfit_host_check.cpp.

A case is a dict: chain (ctypes hrp_fk_chain), pts2d [nkp, 2], K [3, 3], q0 [dof], rot0 [3 | 6], trans0 [3], free (bool [dof]),
free_pose, root, and optionally w2d, pts3d + w3d, lo, hi, prior (None where absent); inputs are fp32 values."""
import ctypes
import struct

import numpy as np

CONVERGED, AT_LIMIT, FEW_ROWS, BAD_START = 1, 2, 4, 8
MAX_IT = 200
OPTIONAL = ("w2d", "pts3d", "w3d", "lo", "hi", "prior")


def tables(chain):
    nj, nkp = int(chain.njoints), int(chain.nkp)
    return dict(nj=nj, nkp=nkp, dof=int(chain.dof), parent=[chain.parent[i] for i in range(nj)], type=[chain.type[i] for i in range(nj)],
                cfg=[chain.cfg[i] for i in range(nj)], mul=[float(chain.mimic_mul[i]) for i in range(nj)],
                off=[float(chain.mimic_off[i]) for i in range(nj)],
                origin=[np.array([chain.origin[i][k] for k in range(12)], dtype=np.float64).reshape(3, 4) for i in range(nj)],
                axis=[np.array([chain.axis[i][k] for k in range(3)], dtype=np.float64) for i in range(nj)],
                kp_frame=[chain.kp_frame[k] for k in range(nkp)],
                kp_offset=[np.array([chain.kp_offset[k][r] for r in range(3)], dtype=np.float64) for k in range(nkp)])


def skew(w):
    return np.array([[0 * w[0], -w[2], w[1]], [w[2], 0 * w[0], -w[0]], [-w[1], w[0], 0 * w[0]]])


def rodrigues(w):
    """R(w), also for a complex w (complex-step derivative): theta = sqrt(w . w) without conjugation."""
    w = np.asarray(w)
    s = (w * w).sum()
    Kx = skew(w)
    if abs(s) < 1e-16:
        return np.eye(3) + Kx + 0.5 * (Kx @ Kx)
    th = np.sqrt(s)
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / s * (Kx @ Kx)


def rot_from_6d(r6):
    a, b = np.asarray(r6[:3], dtype=np.float64), np.asarray(r6[3:], dtype=np.float64)
    x = a / np.linalg.norm(a)
    z = np.cross(x, b)
    z = z / np.linalg.norm(z)
    return np.stack([x, np.cross(z, x), z])


def rotvec(R):
    """Angle-axis of R through its quaternion, |w| <= pi."""
    q = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                  1 - R[0, 0] - R[1, 1] + R[2, 2]])
    i = int(np.argmax(q))
    if i == 0:
        v = np.array([q[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif i == 1:
        v = np.array([R[2, 1] - R[1, 2], q[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif i == 2:
        v = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], q[2], R[1, 2] + R[2, 1]])
    else:
        v = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], q[3]])
    v = v / np.linalg.norm(v)
    if v[0] < 0:
        v = -v
    n = np.linalg.norm(v[1:])
    return np.zeros(3) if n < 1e-300 else 2 * np.arctan2(n, v[0]) / n * v[1:]


def frames(tab, q):
    T = [None] * tab["nj"]
    for j in range(tab["nj"]):
        O = np.eye(4, dtype=q.dtype)
        O[:3] = tab["origin"][j]
        M = np.eye(4, dtype=q.dtype)
        cfg = tab["cfg"][j]
        if tab["type"][j] != 0 and 0 <= cfg < tab["dof"]:
            qv = tab["mul"][j] * q[cfg] + tab["off"][j]
            if tab["type"][j] == 1:
                M[:3, :3] = rodrigues(tab["axis"][j] * qv)
            else:
                M[:3, 3] = tab["axis"][j] * qv
        T[j] = (np.eye(4) if tab["parent"][j] < 0 else T[tab["parent"][j]]) @ O @ M
    return T


def keypoints(tab, q, R, t, root=0):
    """Camera-frame key-points [nkp, 3]: M FK_k(q), M = [R | t] (root == 0) or [R | t] T_root(q)^-1."""
    q = np.asarray(q)
    T = frames(tab, q)
    M = np.eye(4, dtype=np.result_type(q.dtype, np.asarray(R).dtype, np.asarray(t).dtype))
    M[:3, :3], M[:3, 3] = R, t
    if root > 0 and tab["kp_frame"][root] >= 0:
        M = M @ np.linalg.inv(T[tab["kp_frame"][root]])
    out = []
    for k in range(tab["nkp"]):
        F = np.eye(4) if tab["kp_frame"][k] < 0 else T[tab["kp_frame"][k]]
        out.append((M @ F)[:3, :3] @ tab["kp_offset"][k] + (M @ F)[:3, 3])
    return np.array(out)


def project(K, X):
    h = X @ np.asarray(K, dtype=np.float64).T
    return h[:, :2] / h[:, 2:3]


class Problem:
    """A case with everything derived from it: used points, parameter layout, start."""

    def __init__(self, case):
        self.c = c = case
        self.tab = tables(c["chain"])
        self.nkp, self.dof = self.tab["nkp"], self.tab["dof"]
        f64 = lambda v: None if v is None else np.asarray(v, dtype=np.float64)      # noqa: E731
        self.x, self.K, self.q0, self.t0 = f64(c["pts2d"]), f64(c["K"]).reshape(3, 3), f64(c["q0"]), f64(c["trans0"])
        rot0 = f64(c["rot0"])
        self.R0 = rodrigues(rot0) if rot0.size == 3 else rot_from_6d(rot0)
        self.w0 = rot0 if rot0.size == 3 else rotvec(self.R0)
        self.w2d = np.ones(self.nkp) if c.get("w2d") is None else f64(c["w2d"])
        self.Y, self.w3d = f64(c.get("pts3d")), f64(c.get("w3d"))
        self.lo, self.hi, self.prior = f64(c.get("lo")), f64(c.get("hi")), f64(c.get("prior"))
        self.free = np.asarray(c["free"], dtype=bool)
        self.idx = np.flatnonzero(self.free)
        self.free_pose, self.root = bool(c["free_pose"]), int(c["root"])
        self.nfree = len(self.idx)
        self.npar = self.nfree + (6 if self.free_pose else 0)
        with np.errstate(invalid="ignore"):
            self.u2 = (self.w2d > 0) & np.isfinite(self.x).all(1)
            self.u3 = np.zeros(self.nkp, bool) if self.Y is None else (self.w3d > 0) & np.isfinite(self.Y).all(1)
        pr = np.zeros(self.dof) if self.prior is None else np.where(self.prior > 0, self.prior, 0.0)
        self.pw = pr[self.idx]
        self.rows = 2 * int(self.u2.sum()) + 3 * int(self.u3.sum()) + int((self.pw > 0).sum())
        self.p0 = np.concatenate([self.q0[self.idx]] + ([self.w0, self.t0] if self.free_pose else []))
        self.plo = np.full(self.npar, -np.inf)
        self.phi = np.full(self.npar, np.inf)
        if self.lo is not None:
            self.plo[:self.nfree] = self.lo[self.idx]
        if self.hi is not None:
            self.phi[:self.nfree] = self.hi[self.idx]

    def split(self, p):
        p = np.asarray(p)
        q = self.q0.astype(p.dtype)
        q[self.idx] = p[:self.nfree]
        if self.free_pose:
            return q, rodrigues(p[self.nfree:self.nfree + 3]), p[self.nfree + 3:]
        return q, self.R0, self.t0

    def points(self, p):
        q, R, t = self.split(p)
        return keypoints(self.tab, q, R, t, self.root)

    def residuals(self, p):
        """The weighted residual rows of the used points and the priors (their squares sum to C), and the camera depths."""
        X = self.points(p)
        uv = project(self.K, X)
        r = [(np.sqrt(self.w2d[self.u2])[:, None] * (uv[self.u2] - self.x[self.u2])).ravel()]
        if self.u3.any():
            r.append((np.sqrt(self.w3d[self.u3])[:, None] * (X[self.u3] - self.Y[self.u3])).ravel())
        m = self.pw > 0
        r.append(np.sqrt(self.pw[m]) * (np.asarray(p)[:self.nfree][m] - self.q0[self.idx][m]))
        return np.concatenate(r), X[:, 2]

    def cost(self, p):
        """(C, usable): usable is False with a used 2-D point at depth <= 0 or a cost that is not finite."""
        with np.errstate(all="ignore"):
            r, z = self.residuals(p)
            C = float((r * r).sum())
            return C, bool(np.isfinite(C) and (z.real[self.u2] > 0).all())

    def jacobian(self, p, h=1e-30):
        p = np.asarray(p, dtype=np.float64)
        J = np.zeros((len(self.residuals(p)[0]), self.npar))
        for i in range(self.npar):
            pc = p.astype(np.complex128)
            pc[i] += 1j * h
            J[:, i] = self.residuals(pc)[0].imag / h
        return J

    def rms(self, p):
        if not self.u2.any():
            return 0.0
        e = project(self.K, self.points(p))[self.u2] - self.x[self.u2]
        return float(np.sqrt((self.w2d[self.u2] * (e * e).sum(1)).sum() / self.w2d[self.u2].sum()))

    def covariance(self, p):
        J = self.jacobian(p)
        return self.cost(p)[0] / (self.rows - self.npar) * np.linalg.inv(J.T @ J)

    def lm(self):
        """hrp_kin_solve's loop: (p, flags, trials)."""
        p, flags, it = self.p0.copy(), 0, 0
        cost, ok = self.cost(p)
        if self.rows < self.npar or self.npar == 0:
            flags |= FEW_ROWS
        if not ok:
            flags |= BAD_START
        if flags:
            return p, flags, 0

        def lin(p):
            J = self.jacobian(p)
            g = J.T @ self.residuals(p)[0]
            held = ((p <= self.plo) & (g > 0)) | ((p >= self.phi) & (g < 0))
            return J.T @ J, g, held
        M, g, held = lin(p)
        lam, conv = 1e-3, 0
        while it < MAX_IT:
            A = M + lam * np.diag(np.diag(M))
            A[held, :] = 0
            A[:, held] = 0
            A[held, held] = 1
            try:
                np.linalg.cholesky(A)
                step = np.linalg.solve(A, np.where(held, 0.0, -g))
                good = True
            except np.linalg.LinAlgError:
                good = False
            if good:
                pt = np.minimum(np.maximum(p + step, self.plo), self.phi)
                smax, ymax = np.abs(pt - p).max(), np.abs(p).max()
                cn, ok = self.cost(pt)
                if ok and cn < cost:
                    p, cost = pt, cn
                    M, g, held = lin(p)
                    lam = max(lam * 0.1, 1e-12)
                    if smax <= 1e-12 * (1 + ymax):
                        conv, it = 1, it + 1
                        break
                    it += 1
                    continue
            lam *= 10
            if lam > 1e10:
                conv, it = 1, it + 1
                break
            it += 1
        flags |= CONVERGED if conv else 0
        if ((p[:self.nfree] == self.plo[:self.nfree]) | (p[:self.nfree] == self.phi[:self.nfree])).any():
            flags |= AT_LIMIT
        return p, flags, it

    def solution_vector(self, q, rot, trans):
        """The kernel's outputs as a parameter vector (rot in the case's rot_dim)."""
        rot = np.asarray(rot, dtype=np.float64)
        w = rot if rot.size == 3 else rotvec(rot_from_6d(rot))
        return np.concatenate([np.asarray(q, dtype=np.float64)[self.idx]] + ([w, np.asarray(trans, dtype=np.float64)] if self.free_pose else []))


def rotvec_close(a, b):
    """Largest component difference of two angle-axis vectors as rotations (w and its 2 pi complement are the same rotation)."""
    return float(np.abs(rotvec(rodrigues(a) @ rodrigues(b).T)).max())


# ---- tests/kinfit_host_check.cpp's file format ------------------------------------------------------------------------------------------
def pack_case(case):
    P = Problem(case)
    rot0 = np.asarray(case["rot0"], dtype=np.float32).ravel()
    present = sum(1 << i for i, k in enumerate(OPTIONAL) if case.get(k) is not None)
    free_q = sum(1 << int(j) for j in P.idx)
    head = struct.pack("<8i", P.nkp, P.dof, rot0.size, int(P.free_pose), P.root, free_q - (1 << 32) if free_q >= 1 << 31 else free_q, present, 0)
    f32 = lambda v, n: (np.zeros(n, np.float32) if v is None else np.asarray(v, dtype=np.float32).ravel()).tobytes()      # noqa: E731
    body = [bytes(case["chain"]), f32(case["pts2d"], 0), f32(case.get("w2d"), P.nkp), f32(case.get("pts3d"), 3 * P.nkp),
            f32(case.get("w3d"), P.nkp), f32(case["K"], 0), f32(case["q0"], 0), rot0.tobytes(), f32(case["trans0"], 0),
            f32(case.get("lo"), P.dof), f32(case.get("hi"), P.dof), f32(case.get("prior"), P.dof)]
    return head + b"".join(body)


def unpack_results(raw, cases):
    out, off = [], 0
    for case in cases:
        P = Problem(case)
        rd = np.asarray(case["rot0"]).size

        def take(n, dt=np.float32):
            nonlocal off
            a = np.frombuffer(raw[off:off + 4 * n], dt).copy()
            off += 4 * n
            return a
        out.append(dict(q=take(P.dof), rot=take(rd), trans=take(3), rms=take(1)[0], status=take(4, np.int32),
                        xyz=take(3 * P.nkp).reshape(-1, 3), uv=take(2 * P.nkp).reshape(-1, 2), cov=take(P.npar * P.npar).reshape(P.npar, P.npar)))
    assert off == len(raw), (off, len(raw))
    return out


def write_cases(path, cases):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)) + b"".join(pack_case(c) for c in cases))


# ---- chains ---------------------------------------------------------------------------------------------------------------------------------
def point_chain(FkChain, pts):
    """A chain without joints whose key-points are the given points (kp_frame = -1, offsets = the points)."""
    ch = FkChain()
    ch.njoints, ch.dof, ch.nkp = 0, 0, len(pts)
    for k, p in enumerate(pts):
        ch.kp_frame[k] = -1
        for r in range(3):
            ch.kp_offset[k][r] = float(p[r])
    return ch


def serial_chain(FkChain, njoints=32, nkp=24, seed=0):
    """A synthetic serial chain: revolute joints with alternating axes and short offsets, key-points spread along it."""
    rng = np.random.default_rng(seed)
    ch = FkChain()
    ch.njoints = ch.dof = njoints
    axes = [(0, 0, 1), (0, 1, 0), (1, 0, 0)]
    for j in range(njoints):
        ch.parent[j], ch.type[j], ch.cfg[j] = j - 1, 1, j
        ch.mimic_mul[j], ch.mimic_off[j] = 1.0, 0.0
        O = np.eye(4)[:3]
        O[:, 3] = np.float32(0.06 * rng.standard_normal(3) + (0, 0, 0.05))
        for k in range(12):
            ch.origin[j][k] = float(O.ravel()[k])
        for r in range(3):
            ch.axis[j][r] = float(axes[j % 3][r])
    ch.nkp = nkp
    for k in range(nkp):
        ch.kp_frame[k] = min(njoints - 1, (k * njoints) // nkp + (njoints // nkp))
        o = np.float32(0.08 * rng.standard_normal(3))
        for r in range(3):
            ch.kp_offset[k][r] = float(o[r])
    return ch


def chain_from_bytes(FkChain, raw):
    ch = FkChain()
    ctypes.memmove(ctypes.addressof(ch), bytes(raw), ctypes.sizeof(ch))
    return ch


# ---- tests/golden/golden_kinfit.npz ---------------------------------------------------------------------------------------------------------
ROBOTS = ("panda", "kuka", "baxter")
_ORDER = ("pts2d", "w2d", "pts3d", "w3d", "q0", "rot0", "trans0", "lo", "hi", "prior")


def encode_case(name, case, ref):
    P = Problem(case)
    present = sum(1 << i for i, k in enumerate(_ORDER) if case.get(k) is not None)
    meta = [ROBOTS.index(case["robot"]), P.nkp, P.dof, np.asarray(case["rot0"]).size, int(P.free_pose), P.root,
            sum(1 << int(j) for j in P.idx), present, int(ref["flags"]), int(ref["trials"]), int(ref["seed"])]
    return {f"{name}_in": np.concatenate([np.asarray(case[k], dtype=np.float32).ravel() for k in _ORDER if case.get(k) is not None]),
            f"{name}_meta": np.array(meta, dtype=np.int32),
            f"{name}_ref": np.concatenate([[ref["rms"], ref["maxJ"]], ref["p_star"]]).astype(np.float64)}


def load_fixture(path, chain_of):
    """{name: (case, ref)} from golden_kinfit.npz; chain_of(robot name) gives the ctypes chain."""
    g = np.load(path)
    out = {}
    for name in g["cases"]:
        name = str(name)
        m, raw, ref = g[f"{name}_meta"], g[f"{name}_in"], g[f"{name}_ref"]
        robot, nkp, dof, rd, free_pose, root, bits, present, flags, trials, seed = (int(v) for v in m)
        sizes = dict(pts2d=(nkp, 2), w2d=(nkp,), pts3d=(nkp, 3), w3d=(nkp,), q0=(dof,), rot0=(rd,), trans0=(3,), lo=(dof,), hi=(dof,), prior=(dof,))
        case, off = dict(chain=chain_of(ROBOTS[robot]), robot=ROBOTS[robot], K=g["K"], free_pose=bool(free_pose), root=root,
                         free=np.array([bool(bits >> j & 1) for j in range(dof)])), 0
        for i, k in enumerate(_ORDER):
            if present >> i & 1:
                n = int(np.prod(sizes[k]))
                case[k] = raw[off:off + n].reshape(sizes[k]).copy()
                off += n
        assert off == len(raw), name
        out[name] = (case, dict(rms=float(ref[0]), maxJ=float(ref[1]), p_star=ref[2:].copy(), flags=flags, trials=trials, seed=seed))
    return out
