"""The float64 numpy statement of hrp_kin_smooth (include/hrp.h), written from the header's semantics on top of kinfilter_oracle and
shared by tests/golden/gen_golden_kinsmooth.py, tests/test_kinsmooth_host.py and tests/test_gpu_kinsmooth.py.

``rts(hist, q_acc)`` is the Rauch-Tung-Striebel pass over one stream's history, dict(mean [L, 2n], cov [L, 2n, 2n], valid [L], flags [L]
(the filter step's), dt [L]), oldest frame first.  Three formulations of the same recursion: how="chol" (float64, Cholesky of P- and 2n
solves: what the kernel does), how="inv" (float64, the explicit inverse of P-) and dtype=np.longdouble (how="chol" with every operation
in 80-bit arithmetic; the Cholesky and the substitutions are written out here because LAPACK has no such type).  ``own_figures`` is the
larger distance of the two float64 formulations to the 80-bit one: the tests' fp64 gates are ten times that, per case.

``synthetic`` draws a history from a linear-Gaussian toy (a Kalman filter on (p, v) with the filter's own motion model and a constant
H), ``batch_wls`` solves the same toy as one weighted least-squares problem over the whole sequence: the generator pins ``rts`` to it."""
import struct

import numpy as np

import kinfilter_oracle as kf
import kinfit_oracle as ko

SMOOTHED, TAIL, INVALID, BAD_LINK, CLAMPED = 1, 2, 4, 8, 16
CUTS = kf.INIT | kf.BAD_START | kf.REWRAPPED
HAVE_LD = np.finfo(np.longdouble).nmant >= 63


def transition(n, dt, q_acc, dtype=np.float64):
    dt = dtype(dt)
    q = np.asarray(q_acc, dtype)
    I, Z = np.eye(n, dtype=dtype), np.zeros((n, n), dtype)
    F = np.block([[I, dt * I], [Z, I]])
    Q = np.block([[np.diag(q * (dtype(0.25) * dt * dt * dt * dt)), np.diag(q * (dtype(0.5) * dt * dt * dt))],
                  [np.diag(q * (dtype(0.5) * dt * dt * dt)), np.diag(q * (dt * dt))]])
    return F, Q


def chol(A):
    """Lower factor of A in A's dtype, right-looking; None at a pivot that is not positive or not finite."""
    L = np.tril(A).copy()
    N = len(L)
    with np.errstate(all="ignore"):
        for k in range(N):
            d = L[k, k]
            if not (d > 0) or not np.isfinite(d):
                return None
            L[k, k] = np.sqrt(d)
            L[k + 1:, k] = L[k + 1:, k] / L[k, k]
            L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
    return L


def chol_solve(L, Bm):
    """(L L^T)^-1 Bm, column by column, in L's dtype."""
    X = Bm.copy()
    N = len(L)
    for r in range(N):
        X[r] = (X[r] - L[r, :r] @ X[:r]) / L[r, r]
    for r in range(N - 1, -1, -1):
        X[r] = (X[r] - L[r + 1:, r] @ X[r + 1:]) / L[r, r]
    return X


def usable(hist, t):
    with np.errstate(invalid="ignore"):
        return bool(int(hist["valid"][t]) == 1 and np.isfinite(hist["mean"][t]).all() and np.isfinite(np.diag(hist["cov"][t])).all())


def rts(hist, q_acc, how="chol", dtype=np.float64):
    """-> dict(mean [L, 2n], cov [L, 2n, 2n], flags [L] (without CLAMPED), count [L]) in ``dtype``; INVALID frames are zeros."""
    L, N = hist["mean"].shape
    n = N // 2
    xs, Ps = np.zeros((L, N), dtype), np.zeros((L, N, N), dtype)
    flags, count = np.zeros(L, np.int64), np.zeros(L, np.int64)
    for t in range(L - 1, -1, -1):
        if not usable(hist, t):
            flags[t] = INVALID
            continue
        x, P = hist["mean"][t].astype(dtype), hist["cov"][t].astype(dtype)
        G = None
        bad = False
        if t + 1 < L and usable(hist, t + 1) and not int(hist["flags"][t + 1]) & CUTS:
            F, Q = transition(n, hist["dt"][t + 1], q_acc, dtype)
            with np.errstate(all="ignore"):
                Pm = F @ P @ F.T + Q
                Lf = chol(Pm)
                if Lf is not None:
                    G = (P @ F.T) @ np.linalg.inv(Pm) if how == "inv" else chol_solve(Lf, (P @ F.T).T.copy()).T
                    if not np.isfinite(G.astype(np.float64)).all():
                        G = None
            bad = G is None
        if G is None:
            xs[t], Ps[t] = x, P
            flags[t] = TAIL | (BAD_LINK if bad else 0)
        else:
            xs[t] = x + G @ (xs[t + 1] - F @ x)
            S = P + G @ (Ps[t + 1] - Pm) @ G.T
            Ps[t] = np.tril(S) + np.tril(S, -1).T
            flags[t], count[t] = SMOOTHED, count[t + 1] + 1
    return dict(mean=xs, cov=Ps, flags=flags, count=count)


def distance(a, ref):
    """(mean in units of the smoothed standard deviation, covariance relative to sqrt(P_ii P_jj)) of result a against ref."""
    dm = dc = 0.0
    for t in range(len(ref["mean"])):
        if ref["flags"][t] & INVALID:
            continue
        sd = np.sqrt(np.diag(ref["cov"][t]).astype(np.float64))
        dm = max(dm, float(np.abs((a["mean"][t] - ref["mean"][t]).astype(np.float64) / sd).max()))
        dc = max(dc, float((np.abs((a["cov"][t] - ref["cov"][t]).astype(np.float64)) / np.outer(sd, sd)).max()))
    return dm, dc


def own_figures(hist, q_acc):
    """The oracle-alone figures (mean, cov) of a history: the larger distance of the two float64 formulations to the 80-bit one; where
    the host has no 80-bit long double, the distance between the two float64 formulations."""
    a, b = rts(hist, q_acc, "chol"), rts(hist, q_acc, "inv")
    if not HAVE_LD:
        return distance(b, a)
    ref = rts(hist, q_acc, "chol", np.longdouble)
    assert np.array_equal(ref["flags"], a["flags"]) and np.array_equal(ref["flags"], b["flags"])
    return tuple(np.maximum(distance(a, ref), distance(b, ref)))


# ---- the fp32 outputs of a smoothed frame ---------------------------------------------------------------------------------------------------
def outputs(F, xs, q_in, pose_in, rot_dim=3):
    """hrp_kin_smooth's outputs of one usable frame of kinfilter_oracle.Filter F's parameters: dict(q, rot, trans, X, clamped, beyond);
    pose_in = (rot, trans) fp32, the fixed pose when the pose is not free.  beyond: how far the unclamped joints lie outside the bounds
    (> 0) or inside (< 0), per free joint."""
    P, n, nf = F.P, F.n, F.nfree
    p = np.asarray(xs[:n], np.float64).copy()
    pc = p.copy()
    pc[:nf] = np.clip(p[:nf], P.plo[:nf], P.phi[:nf])
    beyond = np.maximum(P.plo[:nf] - p[:nf], p[:nf] - P.phi[:nf])
    P.q0 = np.asarray(q_in, np.float64)
    rot = np.asarray(pose_in[0], np.float64)
    P.R0 = ko.rodrigues(rot) if rot.size == 3 else ko.rot_from_6d(rot)
    P.t0 = np.asarray(pose_in[1], np.float64)
    q, R, t = P.split(pc)
    X = P.points(pc)
    if P.free_pose:
        w = pc[nf:nf + 3].copy()
        th = np.linalg.norm(w)
        if th > np.pi:
            tn = np.fmod(th, 2 * np.pi)
            w *= (tn - 2 * np.pi if tn > np.pi else tn) / th
        rot_out = w if rot_dim == 3 else ko.rodrigues(w)[:2].ravel()
    else:
        rot_out, t = rot, P.t0
    return dict(q=q, rot=rot_out, trans=np.asarray(t, np.float64), X=X, clamped=bool((pc != p).any()), beyond=beyond)


def history_of(states, flags, dts):
    """A history from kinfilter_oracle states (replay's) with the steps' flags and dt."""
    return dict(mean=np.stack([s["mean"] for s in states]), cov=np.stack([s["cov"] for s in states]),
                valid=np.array([int(s["valid"]) for s in states], np.int32), flags=np.asarray(flags, np.int32),
                dt=np.asarray(dts, np.float64))


# ---- a linear-Gaussian toy: the filter's motion model, a constant H on p --------------------------------------------------------------------
def synthetic(n, L, seed, dts=None, q_acc=None, m=None, r=0.05, p0=(0.04, 1.0), return_toy=False):
    """A history [L] of a Kalman filter on (p, v) whose measurements are z = H p + noise, H [m, n] constant; frame 0 is INIT."""
    rng = np.random.default_rng(seed)
    m = n if m is None else m
    dts = np.full(L, 1 / 30) if dts is None else np.asarray(dts, np.float64)
    q_acc = np.full(n, 10.0) if q_acc is None else np.asarray(q_acc, np.float64)
    H = np.concatenate([rng.standard_normal((m, n)) + 2.0 * np.eye(m, n), np.zeros((m, n))], 1)
    x = np.concatenate([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.3, 0.3, n)])
    m0, P0 = np.concatenate([x[:n] + 0.2 * rng.standard_normal(n), np.zeros(n)]), np.diag(np.r_[np.full(n, p0[0]), np.full(n, p0[1])])
    mean, cov, zs = [], [], []
    for t in range(L):
        if t == 0:
            xm, Pm = m0, P0
        else:
            F, Q = transition(n, dts[t], q_acc)
            x = F @ x + np.concatenate([0.5 * dts[t] ** 2 * np.ones(n), dts[t] * np.ones(n)]) * np.tile(np.sqrt(q_acc) * rng.standard_normal(n), 2)
            xm, Pm = F @ mean[-1], F @ cov[-1] @ F.T + Q
        z = H @ x + r * rng.standard_normal(m)
        S = H @ Pm @ H.T + r * r * np.eye(m)
        Kg = Pm @ H.T @ np.linalg.inv(S)
        A = np.eye(2 * n) - Kg @ H
        Pn = A @ Pm @ A.T + r * r * Kg @ Kg.T
        mean.append(xm + Kg @ (z - H @ xm))
        cov.append(0.5 * (Pn + Pn.T))
        zs.append(z)
    hist = dict(mean=np.array(mean), cov=np.array(cov), valid=np.ones(L, np.int32),
                flags=np.array([kf.INIT | kf.CONVERGED] + [kf.CONVERGED] * (L - 1), np.int32), dt=dts.copy())
    if return_toy:
        return hist, q_acc, dict(H=H, z=np.array(zs), r=r, m0=m0, P0=P0)
    return hist, q_acc


def batch_wls(hist, q_acc, toy):
    """The toy's states [L, 2n] as ONE weighted least-squares problem: unknowns x_0 and the accelerations a_1 .. a_{L-1}
    (x_t = F_t x_{t-1} + Gamma_t a_t, a_t ~ N(0, diag(q_acc)), Gamma = [dt^2 / 2 I; dt I]), rows: the prior, the accelerations, z_t."""
    L, N = hist["mean"].shape
    n = N // 2
    nu = N + n * (L - 1)
    # x_t = M_t u, u = (x_0, a_1, ...)
    M = [np.concatenate([np.eye(N), np.zeros((N, nu - N))], 1)]
    for t in range(1, L):
        F, _ = transition(n, hist["dt"][t], q_acc)
        Mt = F @ M[-1]
        Mt[:, N + n * (t - 1):N + n * t] += np.concatenate([0.5 * hist["dt"][t] ** 2 * np.eye(n), hist["dt"][t] * np.eye(n)])
        M.append(Mt)
    rows = [np.diag(1 / np.sqrt(np.diag(toy["P0"]))) @ M[0]]
    rhs = [toy["m0"] / np.sqrt(np.diag(toy["P0"]))]
    rows.append(np.concatenate([np.zeros((nu - N, N)), np.diag(np.tile(1 / np.sqrt(q_acc), L - 1))], 1))
    rhs.append(np.zeros(nu - N))
    for t in range(L):
        rows.append(toy["H"] @ M[t] / toy["r"])
        rhs.append(toy["z"][t] / toy["r"])
    u = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]
    return np.array([Mt @ u for Mt in M])


# ---- the synthetic cases of the tests (tests/golden/gen_golden_kinsmooth.py stores their oracle-alone figures) -------------------------------
def plant(hist, what, t):
    """A cut planted at frame t: 'init' / 'rewrapped' (the step's flag), 'invalid' (valid = 0), 'notpd' (frame t-1's covariance gets a
    correlation of 10 between two rates, so the P- of the link t-1 -> t has a pivot that is not positive; the diagonal stays as it was)."""
    if what == "init":
        hist["flags"][t] |= kf.INIT
    elif what == "rewrapped":
        hist["flags"][t] |= kf.REWRAPPED
    elif what == "invalid":
        hist["valid"][t] = 0
    elif what == "notpd":
        n = hist["mean"].shape[1] // 2
        P = hist["cov"][t - 1]
        P[n, n + 1] = P[n + 1, n] = 10.0 * np.sqrt(P[n, n] * P[n + 1, n + 1])
    return hist


def synthetic_cases():
    """{name: dict(robot, free [dof] bool, free_pose, hist, q_acc, cap, first)}: what tests/test_gpu_kinsmooth.py sends through
    kin_smooth and tests/test_kinsmooth_host.py through the host program.  The robots only supply a chain of the right size."""
    dof = dict(panda=8, baxter=15)
    mask = lambda r, k: np.arange(dof[r]) < k      # noqa: E731
    cases = {}

    def add(name, robot, k, free_pose, L, seed, dts=None, cap=None, first=0, cuts=()):
        n = k + (6 if free_pose else 0)
        hist, q_acc = synthetic(n, L, seed, dts=dts)
        for what, t in cuts:
            plant(hist, what, t)
        cases[name] = dict(robot=robot, free=mask(robot, k), free_pose=free_pose, hist=hist, q_acc=q_acc, cap=L if cap is None else cap, first=first)
    add("n1", "panda", 1, False, 12, 1)
    add("n20", "baxter", 14, True, 8, 2)
    add("L1", "panda", 6, False, 1, 3)
    add("L2", "panda", 6, False, 2, 4)
    add("L33", "panda", 6, False, 33, 5)
    add("wrapped", "panda", 6, True, 12, 6, cap=16, first=11)
    add("cuts", "panda", 6, False, 16, 7, cuts=(("init", 3), ("rewrapped", 6), ("invalid", 9), ("init", 12), ("notpd", 13)))
    add("dt", "panda", 6, False, 10, 8, dts=np.array([1 / 30, 1 / 30, 1 / 15, 1 / 60, 1 / 30, 0.1, 1 / 30, 1 / 120, 1 / 30, 1 / 24]))
    return cases


def in_ring(hist, cap, first):
    """The history laid into a ring of cap slots from slot ``first`` (the other slots hold NaN / garbage that must not be read)."""
    L, N = hist["mean"].shape
    ring = dict(mean=np.full((cap, N), np.nan), cov=np.full((cap, N, N), np.nan), valid=np.full(cap, 7, np.int32), flags=np.full(cap, -1, np.int32),
                dt=np.full(cap, np.nan))
    for t in range(L):
        s = (first + t) % cap
        for k in ring:
            ring[k][s] = hist[k][t]
    return ring


# ---- tests/golden/golden_kinsmooth.npz ---------------------------------------------------------------------------------------------------------
def load_fixture(path):
    """{name: dict(own (mean, cov), flags [L], count [L], ...)} of the golden sequences and the synthetic cases."""
    g = np.load(path)
    out = {}
    for i, name in enumerate(g["names"]):
        a, b = int(g["offsets"][i]), int(g["offsets"][i + 1])
        out[str(name)] = dict(own=g["own"][i], err=g["err"][i], flags=g["flags"][a:b], count=g["count"][a:b], beyond=g["beyond"][i])
    return out


# ---- tests/kinsmooth_host_check.cpp's file format ----------------------------------------------------------------------------------------------
def pack_case(chain, free, free_pose, root, rot_dim, ring, q_in, pose, lo, hi, q_acc, cap, first, L, want_cov):
    """One call of one stream: ring = in_ring's dict, q_in [cap, dof] fp32, pose (rot [rot_dim], trans [3]) or None, lo / hi [dof] or
    None."""
    dof, nkp = int(chain.dof), int(chain.nkp)
    free_q = sum(1 << int(j) for j in np.flatnonzero(free))
    f32 = lambda v: np.asarray(v, dtype=np.float32).ravel().tobytes()      # noqa: E731
    f64 = lambda v: np.asarray(v, dtype=np.float64).ravel().tobytes()      # noqa: E731
    head = struct.pack("<12i", nkp, dof, rot_dim, int(free_pose), root, free_q, int(lo is not None), cap, first, L, int(want_cov), int(pose is not None))
    pose = (np.zeros(rot_dim), np.zeros(3)) if pose is None else pose
    lo = np.zeros(dof) if lo is None else lo
    hi = np.zeros(dof) if hi is None else hi
    return head + b"".join([bytes(chain), f64(ring["mean"]), f64(ring["cov"]), ring["valid"].astype(np.int32).tobytes(),
                            ring["flags"].astype(np.int32).tobytes(), f64(ring["dt"]), f32(q_in), f32(pose[0]), f32(pose[1]), f32(lo), f32(hi),
                            f64(q_acc)])


def unpack_cases(raw, items):
    """items: [(n, dof, nkp, rot_dim, L, want_cov)] -> dicts of the program's outputs per call."""
    out, off = [], 0
    for n, dof, nkp, rd, L, wc in items:
        N = 2 * n

        def take(shape, dt=np.float32):
            nonlocal off
            k = int(np.prod(shape)) * np.dtype(dt).itemsize
            a = np.frombuffer(raw[off:off + k], dt).reshape(shape).copy()
            off += k
            return a
        r = dict(q=take((L, dof)), rot=take((L, rd)), trans=take((L, 3)), vel=take((L, n)), xyz=take((L, nkp, 3)), status=take((L, 2), np.int32),
                 mean=take((L, N), np.float64))
        if wc:
            r["cov"], r["cov_full"] = take((L, n, n)), take((L, N, N), np.float64)
        out.append(r)
    assert off == len(raw), (off, len(raw))
    return out


# ---- the code under test against the oracle: shared by the host and the GPU tests ----------------------------------------------------------------
def check(tag, got, ref, own, F=None, q_in=None, pose=None, rot_dim=3):
    """got: dict(q, rot, trans, vel, xyz | kp3d, status, mean[, cov, cov_full]) of one stream [L, ...] against rts's ``ref``: flags and
    link counts exact, the fp64 mean and covariance within ten times ``own`` = the case's oracle-alone figures, cov_full bit-symmetric,
    vel and cov the roundings of mean and cov_full; with F (a kinfilter_oracle.Filter), q_in [L, dof] and pose also the fp32 outputs: q /
    rot / trans within 1e-5 per component, kp3d within 1e-5, fixed entries bit for bit, CLAMPED where the oracle's value lies beyond a
    bound.  Returns the figures (mean, cov, fp32 parameters, kp3d)."""
    L, N = ref["mean"].shape
    n = N // 2
    xyz = got["xyz"] if "xyz" in got else got["kp3d"]
    flags = got["status"][:, 0]
    assert np.array_equal(flags & ~CLAMPED, ref["flags"]), (tag, flags, ref["flags"])
    assert np.array_equal(got["status"][:, 1], ref["count"]), (tag, got["status"][:, 1], ref["count"])
    g = dict(mean=got["mean"], cov=got["cov_full"] if got.get("cov_full") is not None else ref["cov"], flags=ref["flags"])
    dm, dc = distance(g, ref)
    assert dm <= 10 * own[0] and dc <= 10 * own[1], (tag, (dm, dc), own)
    d32 = dx = 0.0
    for t in range(L):
        if ref["flags"][t] & INVALID:
            assert not any(np.asarray(got[k][t]).any() for k in got if k != "status" and got[k] is not None), tag
            continue
        assert np.array_equal(got["vel"][t], got["mean"][t, n:].astype(np.float32)), tag
        if got.get("cov_full") is not None:
            assert np.array_equal(got["cov_full"][t], got["cov_full"][t].T), tag
            assert np.array_equal(got["cov"][t], got["cov_full"][t, :n, :n].astype(np.float32)), tag
        if ref["flags"][t] & TAIL:
            assert got["mean"][t].tobytes() == ref["mean"][t].tobytes(), tag
            if got.get("cov_full") is not None:
                assert got["cov_full"][t].tobytes() == ref["cov"][t].tobytes(), tag
        if F is None:
            continue
        P, nf = F.P, F.nfree
        o = outputs(F, ref["mean"][t], q_in[t], pose if pose is not None else (np.zeros(3), np.zeros(3)), rot_dim)
        assert ref["flags"][t] & TAIL or nf == 0 or np.abs(o["beyond"]).min() > 1e-9, (tag, t, o["beyond"])      # the decision has a margin
        assert bool(flags[t] & CLAMPED) == o["clamped"], (tag, t, flags[t], o["beyond"])
        assert (got["q"][t][P.idx] <= P.phi[:nf]).all() and (got["q"][t][P.idx] >= P.plo[:nf]).all(), (tag, t)
        assert got["q"][t][~P.free].tobytes() == np.asarray(q_in[t], np.float32)[~P.free].tobytes(), (tag, t)
        if not P.free_pose:
            assert got["rot"][t].tobytes() == np.asarray(pose[0], np.float32).tobytes(), (tag, t)
            assert got["trans"][t].tobytes() == np.asarray(pose[1], np.float32).tobytes(), (tag, t)
        else:
            dr = ko.rotvec_close(P.solution_vector(got["q"][t], got["rot"][t], got["trans"][t])[nf:nf + 3], ko.rotvec(ko.rodrigues(ref["mean"][t][nf:nf + 3])))
            d32 = max(d32, float(np.max(dr)), float(np.abs(got["trans"][t] - o["trans"]).max()))
        d32 = max(d32, float(np.abs(got["q"][t] - o["q"]).max()))
        dx = max(dx, float(np.abs(xyz[t] - o["X"]).max()))
    assert d32 <= 1e-5 and dx <= 1e-5, (tag, d32, dx)
    return dm, dc, d32, dx
