"""The float64 numpy statement of hrp_kin_filter_step (include/hrp.h), written from the header's semantics on top of kinfit_oracle's FK
and shared by tests/golden/gen_golden_kinfilter.py, tests/test_kinfilter_host.py and tests/test_gpu_kinfilter.py.

``Filter.step(state, frame)`` is one frame of one stream.  The update's minimiser comes from scipy ``least_squares`` on the stacked
residual [sqrt(w) e ; sqrt(w_q) (q - q_meas) ; L^-1 (p - p-)] with A = L L^T (the generator), or is GIVEN (``p_plus``): v+ and P+
are closed forms of p+, so the tests rebuild every oracle state from the p+ stored in golden_kinfilter.npz without an optimiser.

state: dict(mean [2n], cov [2n, 2n], valid, coast).  frame: dict(pts2d [nkp, 2], w2d [nkp] | None, q_in [dof], rot_in [3 | 6],
trans_in [3], q_meas [dof] | None, keep), fp32 values."""
import struct

import numpy as np

import kinfit_oracle as ko

INIT, COASTED, LOST, BAD_START, REWRAPPED, CONVERGED, AT_LIMIT = 1, 2, 4, 8, 16, 32, 64
MAX_N = 20
TOL = dict(xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)


def empty_state(n):
    return dict(mean=np.zeros(2 * n), cov=np.zeros((2 * n, 2 * n)), valid=0, coast=0)


class Filter:
    def __init__(self, chain, free, free_pose, root, K, dt, q_acc, p0_var, gate=0.0, max_coast=5, lo=None, hi=None, w_q=None):
        dof, nkp = int(chain.dof), int(chain.nkp)
        case = dict(chain=chain, pts2d=np.zeros((nkp, 2)), K=K, q0=np.zeros(dof), rot0=np.zeros(3), trans0=np.zeros(3), free=free,
                    free_pose=free_pose, root=root, lo=lo, hi=hi)
        self.P = P = ko.Problem(case)
        self.n, self.nfree, self.dof, self.nkp = P.npar, P.nfree, dof, nkp
        self.dt, self.gate, self.max_coast = float(dt), float(gate), int(max_coast)
        self.q_acc, self.p0_var = np.asarray(q_acc, np.float64), np.asarray(p0_var, np.float64)
        assert self.q_acc.shape == (self.n,) and self.p0_var.shape == (2 * self.n,) and 1 <= self.n <= MAX_N
        wq = np.zeros(dof) if w_q is None else np.asarray(w_q, np.float64)
        self.wq = np.where(wq > 0, wq, 0.0)[P.idx]
        self.has_wq = w_q is not None

    # ---- one frame's measurement model ---------------------------------------------------------------------------------------------------
    def _bind(self, fr):
        P = self.P
        f64 = lambda v: np.asarray(v, dtype=np.float64)      # noqa: E731
        P.x, P.q0, P.t0 = f64(fr["pts2d"]), f64(fr["q_in"]), f64(fr["trans_in"])
        rot = f64(fr["rot_in"])
        P.R0 = ko.rodrigues(rot) if rot.size == 3 else ko.rot_from_6d(rot)
        P.w0 = rot if rot.size == 3 else ko.rotvec(P.R0)
        w = np.ones(self.nkp) if fr.get("w2d") is None else f64(fr["w2d"])
        with np.errstate(invalid="ignore"):
            usable = (w > 0) & np.isfinite(w) & np.isfinite(P.x).all(1)
        qm = np.zeros(self.nfree)
        if self.has_wq:
            qm = np.where(self.wq > 0, f64(fr["q_meas"])[P.idx], 0.0)
        p_in = np.concatenate([P.q0[P.idx]] + ([P.w0, P.t0] if P.free_pose else []))
        return w, usable, qm, p_in

    def points(self, p):
        return self.P.points(p)

    def pixel_residuals(self, p, used):
        """(uv - x) of the used points [m, 2] (not weighted) and every point's depth."""
        X = self.P.points(p)
        return ko.project(self.P.K, X)[used] - self.P.x[used], X[:, 2]

    def stacked(self, p, used, w, qm, Linv, pm):
        e, _ = self.pixel_residuals(p, used)
        m = self.wq > 0
        return np.concatenate([(np.sqrt(w[used])[:, None] * e).ravel(), np.sqrt(self.wq[m]) * (np.asarray(p)[:self.nfree][m] - qm[m]),
                               Linv @ (np.asarray(p) - pm)])

    def jac(self, fun, p, h=1e-30):
        p = np.asarray(p, np.float64)
        cols = []
        for i in range(self.n):
            pc = p.astype(np.complex128)
            pc[i] += 1j * h
            cols.append(np.asarray(fun(pc)).imag.ravel() / h)
        return np.stack(cols, 1)

    def usable_start(self, p, usable, w):
        with np.errstate(all="ignore"):
            e, z = self.pixel_residuals(p, usable)
            c = float((w[usable][:, None] * e * e).sum())
            return bool(np.isfinite(c) and np.isfinite(p).all() and (z[usable] > 0).all())

    def predict(self, st):
        n, dt = self.n, self.dt
        m, P = st["mean"], st["cov"]
        pp, vv = np.triu(P[:n, :n]) + np.triu(P[:n, :n], 1).T, np.triu(P[n:, n:]) + np.triu(P[n:, n:], 1).T
        vp = P[n:, :n]
        A = pp + dt * (vp + vp.T) + dt * dt * vv + np.diag(self.q_acc * dt ** 4 / 4)
        B = vp + dt * vv + np.diag(self.q_acc * dt ** 3 / 2)
        C = vv + np.diag(self.q_acc * dt * dt)
        return m[:n] + dt * m[n:], m[n:].copy(), A, B, C

    def minimise(self, fun, pm, second_start=None):
        """scipy's optimum of the stacked residual within the joint bounds (an active bound: the joint is set ON it and the rest solved
        again, as gen_golden_kinfit.py does)."""
        from scipy.optimize import least_squares
        P = self.P
        x0 = pm if second_start is None else second_start
        r = least_squares(fun, x0, jac=lambda z: self.jac(fun, z), method="lm", **TOL)
        p = self.polish(fun, r.x, np.zeros(self.n, bool))
        if ((p < P.plo) | (p > P.phi)).any():
            r = least_squares(fun, np.clip(x0, P.plo + 1e-9, P.phi - 1e-9), jac=lambda z: self.jac(fun, z), bounds=(P.plo, P.phi),
                              method="trf", **TOL)
            p = r.x.copy()
            on_lo, on_hi = np.abs(p - P.plo) < 1e-6, np.abs(p - P.phi) < 1e-6
            fixed = on_lo | on_hi
            p[on_lo], p[on_hi] = P.plo[on_lo], P.phi[on_hi]

            def sub(z):
                full = p.astype(z.dtype)
                full[~fixed] = z
                return fun(full)
            r = least_squares(sub, p[~fixed], jac=lambda z: self.jac(fun, _embed(p, fixed, z))[:, ~fixed],
                              method="lm", **TOL)
            p[~fixed] = r.x
            p = self.polish(fun, p, fixed)
            g = self.jac(fun, p).T @ fun(p)
            assert (g[on_lo] > 0).all() and (g[on_hi] < 0).all() and not ((p < P.plo) | (p > P.phi)).any(), "no KKT point found"
        return p

    def polish(self, fun, p, fixed):
        """Gauss-Newton steps on the parameters that are not fixed, from scipy's answer (MINPACK stops near sqrt(eps)), until the step
        is below 1e-14."""
        p = np.asarray(p, np.float64).copy()
        for _ in range(50):
            J = self.jac(fun, p)[:, ~fixed]
            d = np.linalg.solve(J.T @ J, J.T @ fun(p))
            p[~fixed] -= d
            if np.abs(d).max() < 1e-14:
                break
        return p

    def step(self, st, fr, p_plus=None, second_start=None):
        """-> (new state, out).  out: flags (CONVERGED set on every update), used, gated, d2 [nkp], p, v, A (cov_p), q [dof], w, t, X, uv,
        X_next, p_minus."""
        P, n, nf = self.P, self.n, self.nfree
        w, usable, qm, p_in = self._bind(fr)
        init = (not st["valid"]) or (fr.get("keep", 1) == 0)
        out = dict(d2=np.full(self.nkp, np.nan), used=0, gated=0)
        while True:
            if init:
                pm, vm = p_in.copy(), np.zeros(n)
                A, B, C = np.diag(self.p0_var[:n]), np.zeros((n, n)), np.diag(self.p0_var[n:])
            else:
                pm, vm, A, B, C = self.predict(st)
            with np.errstate(all="ignore"):
                try:
                    L = np.linalg.cholesky(A)
                    ok = bool(np.isfinite(L).all())
                except np.linalg.LinAlgError:
                    ok = False
            ok = ok and self.usable_start(pm, usable, w)
            if ok or init:
                break
            init = True
        flags = INIT if init else 0
        if not ok:
            q, R, t = P.split(p_in)
            X = P.points(p_in)
            out.update(flags=flags | BAD_START, p=p_in, v=np.zeros(n), A=np.zeros((n, n)), q=q, X=X, p_minus=p_in)
            return dict(st, valid=0), out
        Linv, Ainv = np.linalg.inv(L), np.linalg.inv(A)
        used = usable.copy()
        if not init and self.gate > 0 and usable.any():
            e, _ = self.pixel_residuals(pm, usable)
            H = self.jac(lambda z: self.pixel_residuals(z, usable)[0], pm)
            for i, k in enumerate(np.flatnonzero(usable)):
                Hk = H[2 * i:2 * i + 2]
                S = Hk @ A @ Hk.T + np.eye(2) / w[k]
                out["d2"][k] = e[i] @ np.linalg.solve(S, e[i])
            used = usable & ~(out["d2"] > self.gate)
            out["gated"] = int(usable.sum() - used.sum())
        out["p_minus"] = pm

        def finish(p, v, Pn, flags, valid, coast):
            q, R, t = P.split(p)
            X = P.points(p)
            out.update(flags=flags, p=p, v=v, A=Pn[:n, :n], q=q, X=X, uv=ko.project(P.K, X), X_next=P.points(p + self.dt * v))
            return dict(mean=np.concatenate([p, v]), cov=Pn, valid=valid, coast=coast), out

        if not used.any():
            coast = (0 if init else int(st["coast"])) + 1
            lost = coast > self.max_coast
            return finish(pm, vm, np.block([[A, B.T], [B, C]]), flags | COASTED | (LOST if lost else 0), 0 if lost else 1, coast)

        fun = lambda z: self.stacked(z, used, w, qm, Linv, pm)      # noqa: E731
        if isinstance(p_plus, str):          # "polish": Gauss-Newton from p-, for an interior optimum close to it (no scipy)
            p = self.polish(fun, np.clip(pm, P.plo, P.phi), np.zeros(n, bool))
            assert not ((p < P.plo) | (p > P.phi)).any()
        else:
            p = np.asarray(p_plus, np.float64).copy() if p_plus is not None else self.minimise(fun, pm, second_start)
        J = self.jac(fun, p)
        Ap = np.linalg.inv(J.T @ J)
        Ap = 0.5 * (Ap + Ap.T)
        G = B @ Ainv
        v = vm + G @ (p - pm)
        Cn = C - G @ (A - Ap) @ G.T
        Pn = np.block([[Ap, Ap @ G.T], [G @ Ap, 0.5 * (Cn + Cn.T)]])
        flags |= CONVERGED
        if ((p[:nf] == P.plo[:nf]) | (p[:nf] == P.phi[:nf])).any():
            flags |= AT_LIMIT
        out["used"] = int(used.sum())
        out["grad"] = J.T @ fun(p)
        if P.free_pose:
            th = np.linalg.norm(p[nf:nf + 3])
            if th > np.pi:
                tn = np.fmod(th, 2 * np.pi)
                tn = tn - 2 * np.pi if tn > np.pi else tn
                p = p.copy()
                p[nf:nf + 3] *= tn / th
                v[nf:nf + 3] = 0
                r = np.arange(n + nf, n + nf + 3)
                Pn[r, :] = 0
                Pn[:, r] = 0
                Pn[r, r] = self.p0_var[r]
                flags |= REWRAPPED
        return finish(p, v, Pn, flags, 1, 0)


def _embed(p, fixed, z):
    full = p.astype(np.asarray(z).dtype)
    full[~fixed] = z
    return full


def kalman_update(F, st_pred, fr, p_lin, used, w, qm):
    """The textbook EKF update (K = P H^T (H P H^T + R)^-1, Joseph form), linearised at p_lin (the iterated EKF's last iterate), on the
    predicted 2n state (mean (p-, v-), cov): -> (mean, cov).  The measurement is z = (x_used, q_meas), h(p) its prediction."""
    n, nf = F.n, F.nfree
    pm, Pm = st_pred["mean"], st_pred["cov"]
    m = F.wq > 0

    def h(p):
        e, _ = F.pixel_residuals(p, used)
        return np.concatenate([e.ravel(), np.asarray(p)[:nf][m] - qm[m]])      # h(p) - z
    Hp = F.jac(h, p_lin)
    H = np.concatenate([Hp, np.zeros_like(Hp)], 1)
    R = np.diag(np.concatenate([np.repeat(1.0 / w[used], 2), 1.0 / F.wq[m]]))
    S = H @ Pm @ H.T + R
    Kg = Pm @ H.T @ np.linalg.inv(S)
    # iterated EKF: innovation z - h(p_lin) - H (x- - x_lin)
    x_lin = np.concatenate([p_lin, pm[n:]])
    innov = -h(p_lin) - H @ (pm - x_lin)
    mean = pm + Kg @ innov
    IKH = np.eye(2 * n) - Kg @ H
    return mean, IKH @ Pm @ IKH.T + Kg @ R @ Kg.T


# ---- tests/golden/golden_kinfilter.npz -------------------------------------------------------------------------------------------------
ROBOTS = ko.ROBOTS
KINDS = ("smooth", "dropout", "outlier", "limit", "holistic", "restart", "lost")


def sequence_names():
    return [f"{r}_{k}" for r in ROBOTS for k in KINDS if k != "holistic" or r == "panda"]


def load_fixture(path, chain_of):
    """{name: seq}; seq: robot, filter (a Filter), frames (list of frame dicts), p_plus [T, n], flags / used / gated [T], own (the
    oracle-alone figures: teacher-forced and free-running (mean, velocity, covariance))."""
    g = np.load(path)
    out = {}
    for name in g["names"]:
        name = str(name)
        I, f, d = g[f"{name}_i"], g[f"{name}_f"], g[f"{name}_d"]
        robot, free_pose, root, bits, has_w, has_wq, max_coast, T = (int(v) for v in I[:8])
        keep, stt = I[9:9 + T], I[9 + T:].reshape(T, 3)
        chain = chain_of(ROBOTS[robot])
        dof, nkp = int(chain.dof), int(chain.nkp)
        free = np.array([bool(bits >> j & 1) for j in range(dof)])
        n = int(free.sum()) + (6 if free_pose else 0)
        cut = np.cumsum([0, 2, n, 2 * n, dof, dof, dof, 6, 4, T * n])
        (dt, gate), q_acc, p0_var, lo, hi, wq, own, cmp_, p = (d[a:b] for a, b in zip(cut[:-1], cut[1:]))
        assert cut[-1] == len(d), name
        F = Filter(chain, free, bool(free_pose), root, g["K"], dt, q_acc, p0_var, gate, max_coast, lo.astype(np.float32), hi.astype(np.float32),
                   wq.astype(np.float32) if has_wq else None)
        cut = np.cumsum([0, T * nkp * 2, T * nkp if has_w else 0, T * dof, T * 6 if free_pose else 6])
        x, w2d, q_in, pose = (f[a:b] for a, b in zip(cut[:-1], cut[1:]))
        assert cut[-1] == len(f), name
        x, q_in, pose = x.reshape(T, nkp, 2), q_in.reshape(T, dof), pose.reshape(T, 6) if free_pose else pose
        frames = []
        for t in range(T):
            pz = pose[t] if pose.ndim == 2 else pose
            frames.append(dict(pts2d=x[t], w2d=w2d.reshape(T, nkp)[t] if has_w else None, q_in=q_in[t], rot_in=pz[:-3], trans_in=pz[-3:],
                               q_meas=q_in[t] if has_wq else None, keep=int(keep[t])))
        out[name] = dict(robot=ROBOTS[robot], filter=F, frames=frames, p_plus=p.reshape(T, n), flags=stt[:, 0], used=stt[:, 1], gated=stt[:, 2],
                         own=own, cmp=cmp_, shared_pose=pose.ndim == 1)
    return out


def replay(seq):
    """The oracle's free run of a sequence, rebuilt from the stored p+ (no optimiser): [(state, out)] per frame."""
    F, st, res = seq["filter"], empty_state(seq["filter"].n), []
    for t, fr in enumerate(seq["frames"]):
        st, out = F.step(st, fr, p_plus=seq["p_plus"][t])
        res.append((st, out))
    return res


# ---- tests/kinfilter_host_check.cpp's file format ---------------------------------------------------------------------------------------
def pack_step(F, chain, st, fr, chained=False):
    """One step: the settings, the state before it (chained: the program takes the state its previous step left) and the frame."""
    P = F.P
    rot = np.asarray(fr["rot_in"], np.float32).ravel()
    free_q = sum(1 << int(j) for j in P.idx)
    present = (1 if fr.get("w2d") is not None else 0) | (2 if np.isfinite(P.plo[:F.nfree]).any() or np.isfinite(P.phi[:F.nfree]).any() else 0) | \
        (4 if F.has_wq else 0) | (8 if "keep" in fr else 0)
    head = struct.pack("<12i", F.nkp, F.dof, rot.size, int(P.free_pose), P.root, free_q, present, F.max_coast, int(st["valid"]), int(st["coast"]),
                       int(fr.get("keep", 1)), int(chained))
    f32 = lambda v, k: (np.zeros(k, np.float32) if v is None else np.asarray(v, dtype=np.float32).ravel()).tobytes()      # noqa: E731
    f64 = lambda v: np.asarray(v, dtype=np.float64).ravel().tobytes()      # noqa: E731
    lo = np.full(F.dof, -np.inf) if P.lo is None else P.lo
    hi = np.full(F.dof, np.inf) if P.hi is None else P.hi
    wq = np.zeros(F.dof)
    wq[P.idx] = F.wq
    body = [struct.pack("<2d", F.dt, F.gate), bytes(chain), f32(fr["pts2d"], 0), f32(fr.get("w2d"), F.nkp), f32(P.K, 0), f32(fr["q_in"], 0), rot.tobytes(),
            f32(fr["trans_in"], 0), f32(lo, 0), f32(hi, 0), f32(wq, 0), f32(fr.get("q_meas"), F.dof), f64(F.q_acc), f64(F.p0_var), f64(st["mean"]),
            f64(st["cov"])]
    return head + b"".join(body)


def unpack_steps(raw, items):
    """items: [(F, rot_dim)] -> dicts of the program's outputs per step."""
    out, off = [], 0
    for F, rd in items:
        n, nkp, dof = F.n, F.nkp, F.dof

        def take(k, dt=np.float32, size=4):
            nonlocal off
            a = np.frombuffer(raw[off:off + size * k], dt).copy()
            off += size * k
            return a
        out.append(dict(mean=take(2 * n, np.float64, 8), cov=take(4 * n * n, np.float64, 8).reshape(2 * n, 2 * n), valid=take(1, np.int32)[0],
                        coast=take(1, np.int32)[0], status=take(4, np.int32), q=take(dof), rot=take(rd), trans=take(3), xyz=take(3 * nkp).reshape(-1, 3),
                        uv=take(2 * nkp).reshape(-1, 2), vel=take(n), cov_p=take(n * n).reshape(n, n), xyz_next=take(3 * nkp).reshape(-1, 3), d2=take(nkp)))
    assert off == len(raw), (off, len(raw))
    return out


def write_steps(path, steps):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(steps)) + b"".join(steps))


# ---- one step of the code under test against the oracle: shared by the host and the GPU tests ------------------------------------------
def rel_cov(a, b):
    s = np.sqrt(np.outer(np.diag(b), np.diag(b)))
    return float((np.abs(a - b) / s).max())


def check_step(tag, F, fr, got, st, out, own):
    """got: the outputs of one step (mean, cov, valid, coast, status, q, rot, trans, xyz, uv, vel, cov_p, xyz_next, d2) against the
    oracle's (st, out).  The fp32 parameters within 1e-5 per component (the project's kin_solve gate), flags and counts exact, fixed
    entries bit for bit, the fp64 mean, velocity and covariance within ten times ``own`` (the oracle-alone figures (p, v, cov) of
    the sequence).  Returns the figures (fp32 p, fp64 p, v, cov)."""
    P, n, nf = F.P, F.n, F.nfree
    assert int(got["status"][0]) == int(out["flags"]), (tag, got["status"], out["flags"])
    assert (int(got["status"][2]), int(got["status"][3])) == (int(out["used"]), int(out["gated"])), (tag, got["status"])
    assert int(got["valid"]) == int(st["valid"]), tag
    q_in = np.asarray(fr["q_in"], np.float32)
    assert got["q"][~P.free].tobytes() == q_in[~P.free].tobytes(), tag
    if not P.free_pose or out["flags"] & BAD_START:
        assert got["rot"].tobytes() == np.asarray(fr["rot_in"], np.float32).tobytes(), tag
        assert got["trans"].tobytes() == np.asarray(fr["trans_in"], np.float32).tobytes(), tag
    if out["flags"] & BAD_START:
        assert got["q"].tobytes() == q_in.tobytes(), tag
        return 0.0, 0.0, 0.0, 0.0
    assert int(got["coast"]) == int(st["coast"]), tag
    p32 = P.solution_vector(got["q"], got["rot"], got["trans"])
    d32 = np.abs(p32 - out["p"])
    if P.free_pose:
        d32[nf:nf + 3] = ko.rotvec_close(p32[nf:nf + 3], out["p"][nf:nf + 3])
    assert d32.max() <= 1e-5, (tag, d32)
    dp, dv = np.abs(got["mean"][:n] - st["mean"][:n]).max(), np.abs(got["mean"][n:] - st["mean"][n:]).max()
    dc = rel_cov(got["cov"], st["cov"])
    assert dp <= 10 * own[0] and dv <= 10 * own[1] and dc <= 10 * own[2], (tag, (dp, dv, dc), own)
    assert np.array_equal(got["cov"], got["cov"].T), tag
    assert np.array_equal(got["vel"], got["mean"][n:].astype(np.float32)), tag
    assert np.abs(got["xyz"] - out["X"]).max() < 1e-5 and np.abs(got["uv"] - out["uv"]).max() < 1e-2, tag
    assert np.abs(got["xyz_next"] - out["X_next"]).max() < 1e-5, tag
    assert np.abs(got["cov_p"] - out["A"]).max() <= 1e-4 * np.sqrt(np.outer(np.diag(out["A"]), np.diag(out["A"]))).max(), tag
    fin = np.isfinite(out["d2"])
    assert np.array_equal(np.isfinite(got["d2"]), fin), (tag, got["d2"], out["d2"])
    if fin.any():
        assert (np.abs(got["d2"][fin] - out["d2"][fin]) <= 1e-5 * np.maximum(1.0, out["d2"][fin])).all(), (tag, got["d2"], out["d2"])
    return float(d32.max()), float(dp), float(dv), dc
