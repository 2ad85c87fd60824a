"""GPU tests of the kinematic smoother (hrp_kin_history_push and hrp_kin_smooth through kinfit.KinematicFilter.smooth and
kinfit.kin_smooth) against tests/kinsmooth_oracle.py, the float64 numpy statement of include/hrp.h.  The fp64 gates are ten times each
case's own oracle-alone figure (tests/golden/golden_kinsmooth.npz), the fp32 ones the project's 1e-5.  Every launch has B <= 8 and
L <= 33."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import hrpe_amd  # noqa: F401
import kinfilter_oracle as kf
import kinsmooth_oracle as ks
from hrpe_amd import _native as nv
from hrpe_amd.lib.utils import kinfit
from hrpe_amd.lib.utils.urdf_robot import URDFRobot

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_ROBOTS = {}
OUT = ("q", "rot", "trans", "vel", "cov", "kp3d", "status", "mean", "cov_full")


def robot_of(name):
    if name not in _ROBOTS:
        _ROBOTS[name] = URDFRobot(name)
    return _ROBOTS[name]


def make_filter(seq, B, history=0):
    F, fr = seq["filter"], seq["frames"][0]
    P = F.P
    wq = None
    if F.has_wq:
        wq = np.zeros(F.dof)
        wq[P.idx] = F.wq
    flt = kinfit.KinematicFilter(robot_of(seq["robot"]), "holistic" if P.free_pose else "fixed_camera", F.dt, F.q_acc, F.p0_var, streams=B,
                                 cTr=None if P.free_pose else np.concatenate([fr["rot_in"], fr["trans_in"]]).astype(np.float64),
                                 free_joints=P.free, limits=(P.lo, P.hi), gate_chi2=F.gate, max_coast=F.max_coast, w_q=wq,
                                 reference_keypoint_id=P.root)
    flt.history = history
    return flt


def step(flt, seq, frames):
    f32 = lambda k: torch.from_numpy(np.stack([np.asarray(fr[k], np.float32) for fr in frames])).to(DEV)      # noqa: E731
    w2d = None
    if any(fr["w2d"] is not None for fr in frames):
        w2d = torch.from_numpy(np.stack([np.ones(flt.nkp, np.float32) if fr["w2d"] is None else fr["w2d"] for fr in frames])).to(DEV)
    keep = torch.tensor([fr["keep"] for fr in frames], dtype=torch.int32, device=DEV)
    K = torch.from_numpy(np.asarray(seq["filter"].P.K, np.float32)).to(DEV)
    if flt.free_pose:
        return flt.step(f32("pts2d"), K, f32("q_in"), f32("rot_in"), f32("trans_in"), w2d=w2d, keep=keep)
    return flt.step(f32("pts2d"), K, f32("q_in"), w2d=w2d, keep=keep)


def same_bytes(a, b):
    view = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def host(res, b):
    """Stream b of a KinSmoothResult as kinsmooth_oracle.check's dict."""
    return {k: None if v is None else v[:, b].cpu().numpy() for k, v in zip(OUT, res)}


def host_history(h, first, L, b):
    """Stream b of a KinHistory read back, oldest frame first."""
    slots = (first + np.arange(L)) % int(h.mean.shape[0])
    return dict(mean=h.mean[:, b].cpu().numpy()[slots], cov=h.cov[:, b].cpu().numpy()[slots], valid=h.valid[:, b].cpu().numpy()[slots],
                flags=h.flags[:, b].cpu().numpy()[slots], dt=h.dt.cpu().numpy()[slots], q_in=h.q_in[:, b].cpu().numpy()[slots])


@pytest.fixture(scope="module")
def figures():
    return ks.load_fixture(os.path.join(GOLDEN, "golden_kinsmooth.npz"))


@pytest.fixture(scope="module")
def runs():
    """Every golden sequence through the device filter with history = 12, free-running, then smooth(full=True):
    {name: (seq, replay, filter, KinSmoothResult)}; shared and left unchanged."""
    seqs = kf.load_fixture(os.path.join(GOLDEN, "golden_kinfilter.npz"), lambda n: robot_of(n).chain)
    out = {}
    for name, seq in seqs.items():
        flt = make_filter(seq, 1, history=12)
        for fr in seq["frames"]:
            step(flt, seq, [fr])
        out[name] = (seq, kf.replay(seq), flt, flt.smooth(full=True))
    torch.cuda.synchronize()
    return out


def pose_of(seq):
    fr = seq["frames"][0]
    return None if seq["filter"].P.free_pose else (np.asarray(fr["rot_in"], np.float32), np.asarray(fr["trans_in"], np.float32))


def test_end_to_end_on_the_golden_sequences(runs, figures):
    """The smoother alone: against the oracle run on the history the device recorded, read back, at ten times the case's oracle-alone
    figures.  The whole path: against the oracle on kinfilter_oracle.replay's states at ten times the sequence's own free-running filter
    figures (position, rate, covariance).  Status flags and link counts exact both ways."""
    for name, (seq, res, flt, sm) in runs.items():
        F = seq["filter"]
        h, first, L = flt.recorded()
        assert (first, L) == (0, 12) and flt.history == 12
        hist = host_history(h, first, L, 0)
        assert np.array_equal(hist["flags"], [o["flags"] for _, o in res]) and np.array_equal(hist["dt"], np.full(12, F.dt)), name
        assert hist["q_in"].tobytes() == np.stack([fr["q_in"] for fr in seq["frames"]]).astype(np.float32).tobytes(), name
        got = host(sm, 0)
        ref = ks.rts(hist, F.q_acc)
        fig = ks.check(name, got, ref, figures[name]["own"], F, hist["q_in"], pose_of(seq))
        assert np.array_equal(ref["flags"], figures[name]["flags"]) and np.array_equal(ref["count"], figures[name]["count"]), name
        # the whole path
        whole = ks.rts(ks.history_of([s for s, _ in res], [o["flags"] for _, o in res], [F.dt] * 12), F.q_acc)
        own, n = seq["own"][3:], F.n
        ok = ~(whole["flags"] & ks.INVALID).astype(bool)
        dp = np.abs(got["mean"][ok][:, :n] - whole["mean"][ok][:, :n]).max()
        dv = np.abs(got["mean"][ok][:, n:] - whole["mean"][ok][:, n:]).max()
        dc = max(kf.rel_cov(got["cov_full"][t], whole["cov"][t]) for t in np.flatnonzero(ok))
        print(f"{name}: smoother alone fp64 mean {fig[0]:.1e} cov {fig[1]:.1e} (oracle alone {figures[name]['own'][0]:.1e} "
              f"{figures[name]['own'][1]:.1e}), fp32 parameters {fig[2]:.1e} kp3d {fig[3]:.1e}; whole path p {dp:.1e} v {dv:.1e} cov {dc:.1e} "
              f"(filter alone {own[0]:.1e} {own[1]:.1e} {own[2]:.1e})")
        assert dp <= 10 * own[0] and dv <= 10 * own[1] and dc <= 10 * own[2], (name, (dp, dv, dc), own)


def test_synthetic_histories(figures):
    """n = 1 and 2n = 40, L = 1, 2, 33, a wrapped ring, planted cuts (INIT, REWRAPPED, valid = 0, a P- that is not positive definite)
    and a dt that differs per frame, through kin_smooth: flags exact, values within the gates, cov_full bit-symmetric."""
    calls = {}
    for name, c in ks.synthetic_cases().items():
        robot = robot_of(c["robot"])
        L, cap, first = len(c["hist"]["dt"]), c["cap"], c["first"]
        dof = int(robot.chain.dof)
        q_in = np.float32(np.random.default_rng(L).uniform(-1, 1, (L, dof)))
        ring = ks.in_ring(c["hist"], cap, first)
        ring_q = np.full((cap, dof), np.nan, np.float32)
        ring_q[(first + np.arange(L)) % cap] = q_in
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)[:, None]).to(DEV)      # noqa: E731
        h = kinfit.KinHistory(up(ring["mean"]), up(ring["cov"]), up(ring["valid"]), up(ring["flags"]), torch.from_numpy(ring["dt"]).to(DEV), up(ring_q))
        pose = None if c["free_pose"] else (np.float32([0.3, -0.2, 0.1]), np.float32([0.05, -0.1, 1.5]))
        dpose = None if pose is None else tuple(torch.from_numpy(v).to(DEV) for v in pose)
        sm = kinfit.kin_smooth(robot, h, c["q_acc"], c["free"], free_pose=c["free_pose"], pose=dpose, limits=False, first=first, length=L, full=True)
        calls[name] = (c, q_in, pose, sm)
    torch.cuda.synchronize()
    for name, (c, q_in, pose, sm) in calls.items():
        n = len(c["q_acc"])
        F = kf.Filter(robot_of(c["robot"]).chain, c["free"], c["free_pose"], 0, np.eye(3), 1 / 30, c["q_acc"], np.ones(2 * n))
        ref = ks.rts(c["hist"], c["q_acc"])
        assert np.array_equal(ref["flags"], figures[name]["flags"]) and np.array_equal(ref["count"], figures[name]["count"]), name
        fig = ks.check(name, host(sm, 0), ref, figures[name]["own"], F, q_in, pose)
        print(f"{name}: fp64 mean {fig[0]:.1e} cov {fig[1]:.1e} (oracle alone {figures[name]['own'][0]:.1e} {figures[name]['own'][1]:.1e}), "
              f"fp32 parameters {fig[2]:.1e} kp3d {fig[3]:.1e}")
    assert figures["cuts"]["flags"].tolist() == [1, 1, 2, 1, 1, 2, 1, 1, 2, 4, 1, 2, 10, 1, 1, 2]


def test_clamp_on_the_limit_sequences(runs):
    """q <= hi exactly; CLAMPED exactly where the oracle's unclamped value exceeds the bound; mean keeps the unclamped value."""
    for rname in kf.ROBOTS:
        seq, res, flt, sm = runs[f"{rname}_limit"]
        F = seq["filter"]
        P, nf = F.P, F.nfree
        h, first, L = flt.recorded()
        ref = ks.rts(host_history(h, first, L, 0), F.q_acc)
        got = host(sm, 0)
        over = (ref["mean"][:, :nf] > P.phi[:nf]) | (ref["mean"][:, :nf] < P.plo[:nf])
        assert over.any() and np.abs(np.r_[ref["mean"][:11, :nf] - P.phi[:nf], ref["mean"][:11, :nf] - P.plo[:nf]]).min() > 1e-9, rname
        assert (got["q"][:, P.idx] <= P.phi[:nf]).all() and (got["q"][:, P.idx] >= P.plo[:nf]).all(), rname
        assert np.array_equal((got["status"][:, 0] & ks.CLAMPED) != 0, over.any(1)), (rname, got["status"][:, 0], over.any(1))
        assert np.array_equal(got["mean"][:, :nf] > P.phi[:nf], ref["mean"][:, :nf] > P.phi[:nf]), rname
        assert (got["q"][:, P.idx][over] == np.where(ref["mean"][:, :nf] > P.phi[:nf], P.phi[:nf], P.plo[:nf]).astype(np.float32)[over]).all(), rname


def test_determinism_batches_lag_and_cov_off(runs):
    """Two calls return equal bytes; in a mixed batch (smooth, restart, lost, every frame invalid) every stream has the bytes of its
    B = 1 run; smooth(lag=5) is the last five rows of smooth(); cov=False leaves the other outputs' bytes as they are."""
    seq, _, flt, sm = runs["panda_restart"]
    again, last5, nocov = flt.smooth(full=True), flt.smooth(lag=5, full=True), flt.smooth(cov=False, full=True)
    for k, a, b, c, d in zip(OUT, sm, again, last5, nocov):
        assert same_bytes(a, b), k
        assert same_bytes(a[7:], c), k
        if k in ("cov", "cov_full"):
            assert d is None
        else:
            assert same_bytes(a, d), k
    assert flt.smooth(lag=1).status[0, 0].cpu().numpy().tolist() == [ks.TAIL, 0]
    with pytest.raises(nv.HrpError, match="lag"):
        flt.smooth(lag=13)
    names = ["panda_smooth", "panda_restart", "panda_lost"]
    hs = [runs[n][2].recorded()[0] for n in names]
    cat = lambda k: torch.cat([getattr(h, k) for h in hs] + [getattr(hs[0], k)], 1).contiguous()      # noqa: E731
    valid = cat("valid")
    valid[:, 3] = 0
    mixed = kinfit.KinHistory(cat("mean"), cat("cov"), valid, cat("flags"), hs[0].dt, cat("q_in"))
    P = seq["filter"].P
    pose = tuple(torch.from_numpy(v).to(DEV) for v in pose_of(seq))
    kw = dict(free_pose=False, pose=pose, limits=(P.lo, P.hi), full=True)
    batch = kinfit.kin_smooth(robot_of("panda"), mixed, seq["filter"].q_acc, P.free, **kw)
    for b, n in enumerate(names):
        for k, x, y in zip(OUT, batch, runs[n][3]):
            assert same_bytes(x[:, b], y[:, 0]), (n, k)
    one = kinfit.kin_smooth(robot_of("panda"), kinfit.KinHistory(*(v if k == "dt" else v[:, 3:4].contiguous() for k, v in zip(mixed._fields, mixed))),
                            seq["filter"].q_acc, P.free, **kw)
    for k, x, y in zip(OUT, batch, one):
        assert same_bytes(x[:, 3], y[:, 0]), k
        assert k == "status" or not x[:, 3].any(), k
    assert batch.status[:, 3].cpu().numpy().tolist() == [[ks.INVALID, 0]] * 12


def test_recording_moves_nothing_and_refuses_a_graph(runs):
    """With history = T the filter's outputs and state have the bytes of history = 0, frame by frame, also after the ring has wrapped;
    a recording step and smooth raise HrpError while the stream is capturing."""
    seq = runs["panda_outlier"][0]
    plain, rec = make_filter(seq, 1), make_filter(seq, 1, history=5)
    for t, fr in enumerate(seq["frames"]):
        a, b = step(plain, seq, [fr]), step(rec, seq, [fr])
        for k, x, y in zip(a._fields, a, b):
            assert same_bytes(x, y), (t, k)
        for k in ("mean", "cov", "valid", "coast"):
            assert same_bytes(getattr(plain, k), getattr(rec, k)), (t, k)
    h, first, L = rec.recorded()
    assert (first, L) == (12 % 5, 5)
    # the wrapped ring of the last five frames is the tail of the whole sequence's history
    whole = runs["panda_outlier"][2].recorded()[0]
    for k in ("mean", "cov", "valid", "flags", "q_in"):
        assert same_bytes(getattr(h, k)[((first + torch.arange(5)) % 5).to(DEV)], getattr(whole, k)[7:]), k
    full, part = runs["panda_outlier"][3], rec.smooth(full=True)
    for k, x, y in zip(OUT, full, part):
        assert same_bytes(x[7:], y), k
    rec.clear_history()
    assert rec.recorded()[1:] == (0, 0)
    with pytest.raises(nv.HrpError, match="empty"):
        rec.smooth()
    step(rec, seq, [seq["frames"][0]])
    fr = seq["frames"][1]
    pts, q = (torch.from_numpy(np.asarray(fr[k], np.float32)[None]).to(DEV) for k in ("pts2d", "q_in"))
    K = torch.from_numpy(np.asarray(seq["filter"].P.K, np.float32)).to(DEV)
    x = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    raised = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = x + 1
        for call in (lambda: rec.step(pts, K, q), lambda: rec.smooth()):
            try:
                call()
            except nv.HrpError as e:
                raised.append(str(e))
    torch.cuda.synchronize()
    assert len(raised) == 2 and all("graph" in r for r in raised), raised
    assert rec.recorded()[2] == 1 and y.shape == (4,)
