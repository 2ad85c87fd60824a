"""The float64 numpy statement of hrp_kin_solve_views (include/hrp.h), built on tests/kinfit_oracle.py (tables, keypoints, project,
rodrigues) and shared by tests/golden/gen_golden_kinviews.py, tests/test_kinviews_host.py and tests/test_gpu_kinviews.py: the stacked
residual of V views, a complex-step Jacobian, the kernel's LM schedule restated (kinfit_oracle.Problem.lm is the model), rms, rms_view
and the covariance, the packing of a case for tests/kinviews_host_check.cpp and the fixture's format.

A case is a dict: chain (ctypes hrp_fk_chain), pts2d [V, nkp, 2], K [V, 3, 3], poses [V, 6] (angle-axis, translation: camera from
base), q0 [dof], free (bool [dof]), and optionally w2d [V, nkp], lo, hi, prior (None where absent); inputs are fp32 values."""
import struct

import numpy as np

import kinfit_oracle as ko

CONVERGED, AT_LIMIT, FEW_ROWS, BAD_START = ko.CONVERGED, ko.AT_LIMIT, ko.FEW_ROWS, ko.BAD_START
MAX_IT, MAX_VIEWS = ko.MAX_IT, 8
OPTIONAL = ("w2d", "lo", "hi", "prior")

# the cameras of the experiment behind the solver: positions in the base frame (m), all looking at TARGET, base z up
CAMERAS = ((1.5, 0.3, 0.9), (-0.4, 1.5, 0.7), (-1.2, -1.0, 1.2), (0.9, -1.3, 0.5))
TARGET = (0.0, 0.0, 0.4)
K0 = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])


def look_at(position, target=TARGET):
    """cTr [6] of a camera at `position` looking at `target`: x right, y down, z forward."""
    c, z = np.asarray(position, dtype=np.float64), np.asarray(target, dtype=np.float64) - np.asarray(position, dtype=np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x = x / np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.concatenate([ko.rotvec(R), -R @ c])


class Problem:
    """A case with everything derived from it: used points, parameter layout, start."""

    def __init__(self, case):
        self.c = c = case
        self.tab = ko.tables(c["chain"])
        self.nkp, self.dof = self.tab["nkp"], self.tab["dof"]
        f64 = lambda v: None if v is None else np.asarray(v, dtype=np.float64)      # noqa: E731
        self.x, self.q0 = f64(c["pts2d"]), f64(c["q0"])
        self.V = self.x.shape[0]
        self.K, self.poses = f64(c["K"]).reshape(self.V, 3, 3), f64(c["poses"]).reshape(self.V, 6)
        self.R = [ko.rodrigues(w[:3]) for w in self.poses]
        self.t = [w[3:] for w in self.poses]
        self.w2d = np.ones((self.V, self.nkp)) if c.get("w2d") is None else f64(c["w2d"])
        self.lo, self.hi, self.prior = f64(c.get("lo")), f64(c.get("hi")), f64(c.get("prior"))
        self.free = np.asarray(c["free"], dtype=bool)
        self.idx = np.flatnonzero(self.free)
        self.nfree = self.npar = len(self.idx)
        with np.errstate(invalid="ignore"):
            self.u2 = (self.w2d > 0) & np.isfinite(self.x).all(2)
        self.used_view = self.u2.sum(1)
        pr = np.zeros(self.dof) if self.prior is None else np.where(self.prior > 0, self.prior, 0.0)
        self.pw = pr[self.idx]
        self.rows = 2 * int(self.u2.sum()) + int((self.pw > 0).sum())
        self.p0 = self.q0[self.idx].copy()
        self.plo = np.full(self.npar, -np.inf) if self.lo is None else self.lo[self.idx].copy()
        self.phi = np.full(self.npar, np.inf) if self.hi is None else self.hi[self.idx].copy()

    def joints(self, p):
        p = np.asarray(p)
        q = self.q0.astype(p.dtype)
        q[self.idx] = p
        return q

    def points(self, p):
        """Camera-frame key-points of every view [V, nkp, 3]; the forward kinematics runs once."""
        Xb = ko.keypoints(self.tab, self.joints(p), np.eye(3), np.zeros(3))
        return np.stack([Xb @ R.T + t for R, t in zip(self.R, self.t)])

    def reprojection(self, p):
        X = self.points(p)
        return np.stack([ko.project(self.K[v], X[v]) for v in range(self.V)]), X

    def residuals(self, p):
        """The weighted residual rows - views ascending, the used points of each, then the priors - and the camera depths [V, nkp]."""
        uv, X = self.reprojection(p)
        r = [(np.sqrt(self.w2d[v][self.u2[v]])[:, None] * (uv[v][self.u2[v]] - self.x[v][self.u2[v]])).ravel() for v in range(self.V)]
        m = self.pw > 0
        r.append(np.sqrt(self.pw[m]) * (np.asarray(p)[m] - self.q0[self.idx][m]))
        return np.concatenate(r), X[:, :, 2]

    def cost(self, p):
        """(C, usable): usable is False with a used point of any view at depth <= 0 or a cost that is not finite."""
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

    def gradient(self, p):
        return self.jacobian(p).T @ self.residuals(p)[0]

    def rms_view(self, p):
        uv, _ = self.reprojection(p)
        out = np.zeros(self.V)
        for v in range(self.V):
            u = self.u2[v]
            if u.any():
                e = uv[v][u] - self.x[v][u]
                out[v] = np.sqrt((self.w2d[v][u] * (e * e).sum(1)).sum() / self.w2d[v][u].sum())
        return out

    def rms(self, p):
        if not self.u2.any():
            return 0.0
        uv, _ = self.reprojection(p)
        e = uv[self.u2] - self.x[self.u2]
        return float(np.sqrt((self.w2d[self.u2] * (e * e).sum(1)).sum() / self.w2d[self.u2].sum()))

    def covariance(self, p):
        J = self.jacobian(p)
        return self.cost(p)[0] / (self.rows - self.npar) * np.linalg.inv(J.T @ J)

    def lm(self):
        """hrp_kin_solve_views' loop: (p, flags, trials)."""
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
            return J.T @ J, g, ((p <= self.plo) & (g > 0)) | ((p >= self.phi) & (g < 0))
        M, g, held = lin(p)
        lam, conv = 1e-3, 0
        while it < MAX_IT:
            A = M + lam * np.diag(np.diag(M))
            A[held, :] = 0
            A[:, held] = 0
            A[held, held] = 1
            try:
                np.linalg.cholesky(A)
                step, good = np.linalg.solve(A, np.where(held, 0.0, -g)), True
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
                    it += 1
                    if smax <= 1e-12 * (1 + ymax):
                        conv = 1
                        break
                    continue
            lam *= 10
            it += 1
            if lam > 1e10:
                conv = 1
                break
        flags |= CONVERGED if conv else 0
        if ((p == self.plo) | (p == self.phi)).any():
            flags |= AT_LIMIT
        return p, flags, it


def permuted(case, order):
    """The case with its views in another order."""
    order = list(order)
    out = dict(case)
    for k in ("pts2d", "K", "poses", "w2d"):
        if case.get(k) is not None:
            out[k] = np.ascontiguousarray(np.asarray(case[k])[order])
    return out


def ring_of_cameras(V, radius=3.5, target=(0.0, 0.0, 0.8)):
    """V cameras on a circle around the base at alternating heights, all looking at `target`: poses [V, 6]."""
    a = 2 * np.pi * (np.arange(V) + 0.25) / max(V, 1)
    return np.stack([look_at((radius * np.cos(t), radius * np.sin(t), 0.5 + 0.4 * (i % 3)), target) for i, t in enumerate(a)])


def synthetic_case(ch, V, free=None, seed=3):
    """A well-posed problem on a bare chain (kinfit_oracle.serial_chain): exact projections of a planted state into a ring of V cameras,
    the start 0.05 rad off, a prior on every joint."""
    rng = np.random.default_rng(seed)
    tab = ko.tables(ch)
    dof, nkp = tab["dof"], tab["nkp"]
    q = np.float32(0.4 * rng.standard_normal(dof))
    free = np.ones(dof, bool) if free is None else np.asarray(free, bool)
    case = dict(chain=ch, K=np.repeat(np.float32(K0)[None], V, 0), poses=np.float32(ring_of_cameras(V)), q0=q, free=free,
                pts2d=np.zeros((V, nkp, 2), np.float32), prior=np.full(dof, 1.0, np.float32), lo=np.full(dof, -3.0, np.float32),
                hi=np.full(dof, 3.0, np.float32))
    case["pts2d"] = np.float32(Problem(case).reprojection(q.astype(np.float64)[free])[0])
    case["q0"] = np.float32(q + 0.05 * rng.standard_normal(dof) * free)
    return case, Problem(case)


# ---- tests/kinviews_host_check.cpp's file format ----------------------------------------------------------------------------------------
def pack_case(case):
    P = Problem(case)
    present = sum(1 << i for i, k in enumerate(OPTIONAL) if case.get(k) is not None)
    free_q = sum(1 << int(j) for j in P.idx)
    head = struct.pack("<8i", P.nkp, P.dof, P.V, free_q - (1 << 32) if free_q >= 1 << 31 else free_q, present, 0, 0, 0)
    f32 = lambda v, n: (np.zeros(n, np.float32) if v is None else np.asarray(v, dtype=np.float32).ravel()).tobytes()      # noqa: E731
    body = [bytes(case["chain"]), f32(case["pts2d"], 0), f32(case.get("w2d"), P.V * P.nkp), f32(case["K"], 0), f32(case["poses"], 0),
            f32(case["q0"], 0), f32(case.get("lo"), P.dof), f32(case.get("hi"), P.dof), f32(case.get("prior"), P.dof)]
    return head + b"".join(body)


def unpack_results(raw, cases):
    out, off = [], 0
    for case in cases:
        P = Problem(case)

        def take(n, dt=np.float32):
            nonlocal off
            a = np.frombuffer(raw[off:off + 4 * n], dt).copy()
            off += 4 * n
            return a
        out.append(dict(q=take(P.dof), rms=take(1)[0], rms_view=take(P.V), status=take(4, np.int32), used_view=take(P.V, np.int32),
                        xyz=take(3 * P.V * P.nkp).reshape(P.V, -1, 3), uv=take(2 * P.V * P.nkp).reshape(P.V, -1, 2),
                        cov=take(P.npar * P.npar).reshape(P.npar, P.npar)))
    assert off == len(raw), (off, len(raw))
    return out


def write_cases(path, cases):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)) + b"".join(pack_case(c) for c in cases))


# ---- tests/golden/golden_kinviews.npz ---------------------------------------------------------------------------------------------------
ROBOTS = ko.ROBOTS
KINDS = ("v2", "v3", "v4", "occluded", "occluded_view", "weights", "limit", "prior", "shared_vs_per_sample")
_ORDER = ("pts2d", "w2d", "q0", "lo", "hi", "prior")


def encode_case(name, case, ref):
    P = Problem(case)
    present = sum(1 << i for i, k in enumerate(_ORDER) if case.get(k) is not None)
    meta = [ROBOTS.index(case["robot"]), P.nkp, P.dof, P.V, sum(1 << int(j) for j in P.idx), present, int(ref["flags"]), int(ref["trials"]),
            int(ref["seed"])]
    return {f"{name}_in": np.concatenate([np.asarray(case[k], dtype=np.float32).ravel() for k in _ORDER if case.get(k) is not None]),
            f"{name}_meta": np.array(meta, dtype=np.int32),
            f"{name}_ref": np.concatenate([[ref["rms"], ref["grad"], ref["cov_own"]], ref["rms_view"], ref["p_star"]]).astype(np.float64)}


def load_fixture(path, chain_of):
    """({name: (case, ref)}, experiment) from golden_kinviews.npz; chain_of(robot name) gives the ctypes chain.  The views of a case are
    the first V of the file's cameras (``poses`` [4, 6] fp32, ``K`` [3, 3] for every view)."""
    g = np.load(path)
    out = {}
    for name in g["cases"]:
        name = str(name)
        m, raw, ref = g[f"{name}_meta"], g[f"{name}_in"], g[f"{name}_ref"]
        robot, nkp, dof, V, bits, present, flags, trials, seed = (int(v) for v in m)
        sizes = dict(pts2d=(V, nkp, 2), w2d=(V, nkp), q0=(dof,), lo=(dof,), hi=(dof,), prior=(dof,))
        case, off = dict(chain=chain_of(ROBOTS[robot]), robot=ROBOTS[robot], K=np.repeat(g["K"][None], V, 0).copy(), poses=g["poses"][:V].copy(),
                         free=np.array([bool(bits >> j & 1) for j in range(dof)])), 0
        for i, k in enumerate(_ORDER):
            if present >> i & 1:
                n = int(np.prod(sizes[k]))
                case[k] = raw[off:off + n].reshape(sizes[k]).copy()
                off += n
        assert off == len(raw), name
        out[name] = (case, dict(rms=float(ref[0]), grad=float(ref[1]), cov_own=float(ref[2]), rms_view=ref[3:3 + V].copy(),
                                p_star=ref[3 + V:].copy(), flags=flags, trials=trials, seed=seed))
    return out, {str(r): g[f"experiment_{r}"] for r in ROBOTS}
