"""GPU tests of the kinematic refit (hrp_kin_solve through kinfit.kin_solve, and the tracker hook) against tests/kinfit_oracle.py, the
float64 numpy statement of include/hrp.h, and the scipy optima of tests/golden/golden_kinfit.npz.  Every launch has B <= 8."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import hrpe_amd  # noqa: F401
import kinfit_oracle as ko
from hrpe_amd import _native as nv
from hrpe_amd.lib.utils import kinfit
from hrpe_amd.lib.utils.BPnP import pnp_solve
from hrpe_amd.lib.utils.urdf_robot import URDFRobot

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_ROBOTS = {}


def robot_of(name):
    if name not in _ROBOTS:
        _ROBOTS[name] = URDFRobot(name)
    return _ROBOTS[name]


class ChainRobot:
    """What kin_solve reads of a robot, around a bare chain."""
    robot_type = None

    def __init__(self, chain):
        self.chain, self._dev = chain, {}

    def chain_on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.frombuffer(bytearray(bytes(self.chain)), dtype=torch.uint8).to(device)
        return self._dev[key]


def dev(a, B=None):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t if B is None else t.unsqueeze(0).repeat(B, *([1] * t.dim())).contiguous()


def solve(case, robot=None, B=1, shared_pose=False, shared_K=True, **over):
    """kin_solve on B copies of a case."""
    robot = robot or (robot_of(case["robot"]) if case.get("robot") else ChainRobot(case["chain"]))
    opt = lambda k: None if case.get(k) is None else dev(case[k], B)      # noqa: E731
    kw = dict(free_joints=np.asarray(case["free"], bool), free_pose=bool(case["free_pose"]), root=int(case["root"]), w2d=opt("w2d"),
              pts3d=opt("pts3d"), w3d=opt("w3d"), prior_q=case.get("prior"),
              limits=False if case.get("lo") is None else (case["lo"], case["hi"]))
    kw.update(over)
    return kinfit.kin_solve(robot, dev(case["pts2d"], B), dev(case["K"]) if shared_K else dev(case["K"], B), dev(case["q0"], B),
                            dev(case["rot0"]) if shared_pose else dev(case["rot0"], B),
                            dev(case["trans0"]) if shared_pose else dev(case["trans0"], B), **kw)


def host(res, b=0):
    return {k: getattr(res, k)[b].cpu().numpy() for k in res._fields}


def same_bytes(a, b):
    return all(torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)) for k in a._fields)


def param_error(P, p, p_ref):
    d = np.abs(p - p_ref)
    if P.free_pose:
        d[P.nfree:P.nfree + 3] = ko.rotvec_close(p[P.nfree:P.nfree + 3], p_ref[P.nfree:P.nfree + 3])
    return d


@pytest.fixture(scope="module")
def fixture_results():
    cases = ko.load_fixture(os.path.join(GOLDEN, "golden_kinfit.npz"), lambda n: robot_of(n).chain)
    res = {name: solve(case) for name, (case, _) in cases.items()}
    torch.cuda.synchronize()
    return cases, {name: host(r) for name, r in res.items()}


def test_every_fixture_case(fixture_results):
    """|p_dev - p*| <= 1e-5 per component (rad, m), the planted flags, rms within 1e-4 px of the oracle's at p* (the kernel takes rms
    from its fp64 parameters, before they are rounded to fp32)."""
    cases, got = fixture_results
    for name, (case, ref) in cases.items():
        P, r = ko.Problem(case), got[name]
        p = P.solution_vector(r["q"], r["rot"], r["trans"])
        d = param_error(P, p, ref["p_star"])
        print(f"{name}: max |p - p*| {d.max():.2e}, LM trials {r['status'][1]} (oracle {ref['trials']}), rms {r['rms']:.6f} vs {ref['rms']:.6f}")
        assert d.max() <= 1e-5, (name, d)
        assert r["status"][0] == ref["flags"] and r["status"][2] == P.rows and r["status"][3] == P.npar, (name, r["status"])
        assert abs(float(r["rms"]) - ref["rms"]) <= 1e-4, name
        fixed = ~P.free
        assert r["q"][fixed].tobytes() == np.asarray(case["q0"], np.float32)[fixed].tobytes(), name
        if not P.free_pose:
            assert r["rot"].tobytes() == case["rot0"].tobytes() and r["trans"].tobytes() == case["trans0"].tobytes(), name
        X = P.points(p)
        assert np.abs(r["kp3d"] - X).max() < 1e-5 and np.abs(r["kp2d"] - ko.project(P.K, X)).max() < 1e-2, name


def test_covariance(fixture_results):
    """cov against numpy's s^2 inv(J^T J) from a complex-step Jacobian at the RETURNED (fp32) solution, the deviation relative to
    sqrt(cov_ii cov_jj).  The gate of a case is ten times the deviation of the oracle alone: the numpy covariance at p* rounded to fp32
    against the one at p*.  (Where the projections are exact, C at the optimum is rounding noise and both deviations are of order one;
    everywhere else they are ~1e-6.)  All zeros on ``limit``."""
    cases, got = fixture_results
    worst = {}
    for name, (case, ref) in cases.items():
        P, r = ko.Problem(case), got[name]
        if name.endswith("_limit"):
            assert not r["cov"].any(), name
            continue
        rel = lambda a, b: float((np.abs(a - b) / np.sqrt(np.outer(np.diag(b), np.diag(b)))).max())      # noqa: E731
        own = rel(P.covariance(ref["p_star"].astype(np.float32).astype(np.float64)), P.covariance(ref["p_star"]))
        p = P.solution_vector(r["q"], r["rot"], r["trans"])
        if P.free_pose and r["rot"].size == 3:
            p[P.nfree:P.nfree + 3] = r["rot"]
        dev_ = rel(r["cov"].astype(np.float64), P.covariance(p))
        kind = "exact" if name.endswith("_qonly") else "noisy"
        worst[kind] = np.maximum(worst.get(kind, (0.0, 0.0)), (own, dev_))
        print(f"{name}: oracle alone {own:.2e}, device {dev_:.2e}")
        assert dev_ <= 10 * own, (name, dev_, own)
        assert np.array_equal(r["cov"], r["cov"].T) or np.abs(r["cov"] - r["cov"].T).max() <= 1e-6 * np.abs(r["cov"]).max(), name
    print("largest (oracle alone, device):", {k: (f"{v[0]:.2e}", f"{v[1]:.2e}") for k, v in worst.items()})


def test_pose_only_matches_pnp_solve():
    """free_q = 0, free_pose = 1, root = 0, weights 1, rot_dim = 3 on golden_pnp.npz through a chain whose key-points are the fixture's
    3-D points: the same objective and schedule as pnp_solve(ini_pose=...), only the summation order differs - 1e-5, the project's gate
    for a pose (tests/test_gpu_pnp_pooled.py::_close)."""
    g = np.load(os.path.join(GOLDEN, "golden_pnp.npz"))
    runs = []
    for c in g["cases"]:
        x, X, K, Pt = (g[f"{c}_{k}"].astype(np.float32) for k in ("pts2d", "pts3d", "K", "P6d_true"))
        ini = (Pt + np.float32(0.03) * np.float32([1, -1, 1, -1, 1, -1])).astype(np.float32)
        groups = [(slice(0, len(x)), X)] if X.ndim == 2 else [(slice(b, b + 1), X[b]) for b in range(len(x))]
        for sl, pts in groups:
            n = len(pts)
            case = dict(chain=ko.point_chain(nv.FkChain, pts), pts2d=x[sl][0], K=K, q0=np.zeros(0, np.float32), rot0=ini[sl][0, :3],
                        trans0=ini[sl][0, 3:], free=np.zeros(0, bool), free_pose=True, root=0)
            B = len(x[sl])
            res = kinfit.kin_solve(ChainRobot(case["chain"]), dev(x[sl]), dev(K), torch.zeros(B, 0, device=DEV), dev(ini[sl][:, :3]),
                                   dev(ini[sl][:, 3:]), free_joints=np.zeros(0, bool), free_pose=True, limits=False)
            P6, st, rms = pnp_solve(dev(x[sl]), dev(pts) if X.ndim == 2 else dev(pts[None]), dev(K), ini_pose=dev(ini[sl]))
            runs.append((str(c), n, res, P6, st, rms))
    torch.cuda.synchronize()
    worst = 0.0
    for c, n, res, P6, st, rms in runs:
        got = torch.cat([res.rot, res.trans], 1).cpu().numpy().astype(np.float64)
        want = P6.cpu().numpy().astype(np.float64)
        for b in range(len(got)):
            d = max(ko.rotvec_close(got[b, :3], want[b, :3]), np.abs(got[b, 3:] - want[b, 3:]).max())
            worst = max(worst, d)
            assert d < 1e-5, (c, b, got[b], want[b])
        assert (res.status[:, 0].cpu().numpy() & ko.CONVERGED).all() and (res.status[:, 2].cpu().numpy() == 2 * n).all(), c
        assert np.abs(res.rms.cpu().numpy() - rms.cpu().numpy()).max() < 1e-4, c
    print(f"pose only against pnp_solve: largest difference {worst:.2e}")


def test_shared_pose_and_shared_K_give_the_same_bytes(fixture_results):
    cases, _ = fixture_results
    case, _ = cases["kuka_qonly_noise"]
    for B in (1, 3):
        a = solve(case, B=B, shared_pose=True, shared_K=True)
        b = solve(case, B=B, shared_pose=False, shared_K=True)
        c = solve(case, B=B, shared_pose=False, shared_K=False)
        assert a.rot.shape == (B, 3) and same_bytes(a, b) and same_bytes(b, c), B
        assert all(torch.equal(a.q[0], a.q[i]) for i in range(B))
    both, _ = cases["panda_both_prior"]
    assert same_bytes(solve(both, B=3, shared_K=True), solve(both, B=3, shared_K=False))


def test_one_free_parameter(fixture_results):
    cases, _ = fixture_results
    case, ref = cases["panda_qonly"]
    P = ko.Problem(case)
    q_star = P.split(ref["p_star"])[0]
    one = dict(case, q0=np.float32(np.where(np.arange(8) == 3, case["q0"], q_star)), free=np.arange(8) == 3)
    r = host(solve(one))
    torch.cuda.synchronize()
    pl, flags, _ = ko.Problem(one).lm()
    assert list(r["status"][2:]) == [14, 1] and r["status"][0] == flags == ko.CONVERGED and r["cov"].shape == (1, 1) and r["cov"][0, 0] > 0
    assert abs(float(r["q"][3]) - pl[0]) <= 1e-5 and abs(pl[0] - q_star[3]) < 1e-4
    assert np.delete(r["q"], 3).tobytes() == np.delete(one["q0"], 3).tobytes()


def synthetic_case(ch, seed=3):
    """A well-posed npar = 38 problem: exact projections and 3-D targets of a planted state, a prior on every joint."""
    rng = np.random.default_rng(seed)
    tab = ko.tables(ch)
    dof, nkp = tab["dof"], tab["nkp"]
    q = 0.4 * rng.standard_normal(dof)
    pose = np.array([0.4, -0.3, 0.2, 0.05, -0.1, 1.8])
    K = np.float32([[600, 0, 320], [0, 600, 240], [0, 0, 1]])
    X = ko.keypoints(tab, np.float32(q).astype(np.float64), ko.rodrigues(pose[:3]), pose[3:])
    case = dict(chain=ch, pts2d=np.float32(ko.project(K, X)), K=K, q0=np.float32(q + 0.05 * rng.standard_normal(dof)),
                rot0=np.float32(pose[:3] + 0.02 * rng.standard_normal(3)), trans0=np.float32(pose[3:] + 0.02 * rng.standard_normal(3)),
                pts3d=np.float32(X), w3d=np.full(nkp, 1e4, np.float32), prior=np.full(dof, 1.0, np.float32),
                lo=np.full(dof, -3.0, np.float32), hi=np.full(dof, 3.0, np.float32), free=np.ones(dof, bool), free_pose=True, root=0)
    return case, ko.Problem(case)


def test_largest_problem_against_the_numpy_loop():
    """npar = 38 (32 joints and the pose) on a synthetic serial chain with 24 key-points and 3-D targets: every LDS array at its
    largest size, against the numpy restatement of the loop."""
    case, P = synthetic_case(ko.serial_chain(nv.FkChain))
    r = host(solve(case, B=2), 1)
    torch.cuda.synchronize()
    pl, flags, it = P.lm()
    p = P.solution_vector(r["q"], r["rot"], r["trans"])
    d = param_error(P, p, pl)
    print(f"npar {P.npar}, rows {P.rows}: device trials {r['status'][1]}, numpy trials {it}, max |p - p_numpy| {d.max():.2e}")
    assert list(r["status"][2:]) == [152, 38] and r["status"][0] == flags and flags & ko.CONVERGED
    assert d.max() <= 1e-5 and r["cov"].shape == (38, 38) and (np.diag(r["cov"]) > 0).all()


def test_rows_equal_npar_and_one_fewer(fixture_results):
    """rows == npar solves, with cov zero; rows == npar - 1 is FEW_ROWS and the outputs are the start bit for bit."""
    cases, _ = fixture_results
    case, _ = cases["panda_both_q1fixed"]          # npar 11
    w = np.zeros(7, np.float32)
    w[:5] = 1.0
    a = host(solve(dict(case, w2d=w, prior=np.float32([0, 1, 0, 0, 0, 0, 0, 0]))))          # 10 + 1 rows
    b = host(solve(dict(case, w2d=w)))                                                      # 10 rows
    torch.cuda.synchronize()
    assert list(a["status"][2:]) == [11, 11] and not a["status"][0] & (ko.FEW_ROWS | ko.BAD_START) and a["status"][1] > 0 and not a["cov"].any()
    assert list(b["status"]) == [ko.FEW_ROWS, 0, 10, 11] and not b["cov"].any()
    for k, k0 in (("q", "q0"), ("rot", "rot0"), ("trans", "trans0")):
        assert b[k].tobytes() == np.asarray(case[k0], np.float32).tobytes(), k


def test_rot_dim_6_in_and_out(fixture_results):
    """The same pose as two rows of R: the poses agree within 1e-6 after conversion, the joints within 1e-6."""
    cases, got = fixture_results
    for name in ("panda_root3", "baxter_both_prior"):          # baxter: nkp = 17
        case, _ = cases[name]
        R0 = ko.rodrigues(case["rot0"].astype(np.float64))
        r6 = host(solve(dict(case, rot0=np.float32(R0[:2].ravel()))))
        torch.cuda.synchronize()
        r3 = got[name]
        assert r6["rot"].shape == (6,) and r6["status"][0] == r3["status"][0]
        R6, R3 = ko.rot_from_6d(r6["rot"].astype(np.float64)), ko.rodrigues(r3["rot"].astype(np.float64))
        assert np.abs(ko.rotvec(R6 @ R3.T)).max() < 1e-6 and np.abs(r6["trans"] - r3["trans"]).max() < 1e-6, name
        assert np.abs(r6["q"] - r3["q"]).max() < 1e-6 and abs(float(r6["rms"] - r3["rms"])) < 1e-4, name
        assert np.abs(np.linalg.norm(r6["rot"].reshape(2, 3), axis=1) - 1).max() < 1e-6


def test_two_calls_and_a_graph_replay_return_the_same_bytes(fixture_results):
    cases, _ = fixture_results
    case, _ = cases["baxter_with3d"]
    robot = robot_of("baxter")
    args = [dev(case["pts2d"], 4), dev(case["K"]), dev(case["q0"], 4), dev(case["rot0"], 4), dev(case["trans0"], 4)]
    kw = dict(free_joints=case["free"], free_pose=True, pts3d=dev(case["pts3d"], 4), w3d=dev(case["w3d"], 4), prior_q=case["prior"],
              limits=(case["lo"], case["hi"]))
    a = kinfit.kin_solve(robot, *args, **kw)
    b = kinfit.kin_solve(robot, *args, **kw)
    torch.cuda.synchronize()
    assert same_bytes(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        kinfit.kin_solve(robot, *args, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = kinfit.kin_solve(robot, *args, **kw)
    for t in c:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bytes(a, c)


# ---- the tracker hook -----------------------------------------------------------------------------------------------------------------------
H, W = 480, 640


def stub_model(out):
    return lambda reg, root, k_values, K: out


def tracker_scene(case, p_true, root):
    """(tuple a stub model returns, true camera-frame key-points): the regressor's output is the case's start, kp3d_int the truth."""
    P = ko.Problem(case)
    X = np.float32(P.points(p_true))
    q0, R0 = np.float32(case["q0"]), ko.rodrigues(case["rot0"].astype(np.float64))
    xyz_fk = np.float32(ko.keypoints(P.tab, q0.astype(np.float64), R0, case["trans0"].astype(np.float64), root))
    z = lambda *s: torch.zeros(1, *s, device=DEV)      # noqa: E731
    return (dev(q0, 1), dev(np.float32(R0[:2].ravel()), 1), dev(case["trans0"], 1), z(2), z(1), z(7, 3), dev(X, 1), dev(xyz_fk, 1)), X


def test_tracker_holistic_refit_lands_on_the_oracle_optimum(fixture_results):
    from hrpe_amd.lib.core.tracker import PoseTracker
    cases, _ = fixture_results
    case, ref = cases["panda_root3"]
    panda = robot_of("panda")
    out, X = tracker_scene(case, ref["p_star"], 3)
    frames = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    refit = kinfit.KinematicRefit(panda, "holistic", prior_q=1.0)
    plain = PoseTracker(stub_model(out), panda, case["K"], (H, W))
    none = PoseTracker(stub_model(out), panda, case["K"], (H, W), refit=None)
    trk = PoseTracker(stub_model(out), panda, case["K"], (H, W), refit=refit)
    r0, r1, r2 = plain.step(frames), none.step(frames), trk.step(frames)
    torch.cuda.synchronize()
    for a, b in zip(r0, r1):          # refit=None: the bytes of a tracker built without the argument
        assert torch.equal(a, b)
    assert none.refit_result is None and torch.equal(plain.kp2d, none.kp2d)
    K_crop = trk.other_K[0].cpu().numpy()
    x = np.float32(ko.project(K_crop, X.astype(np.float64)))
    obs = kinfit.observable_joints(panda)
    P = ko.Problem(dict(case, pts2d=x, K=K_crop, rot0=out[1][0].cpu().numpy(), free=obs,
                        prior=np.where(obs, 1.0, 0.0).astype(np.float32)))
    p, flags, _ = P.lm()
    want = ko.project(case["K"], P.points(p))
    got, before = r2.kp2d_original[0].cpu().numpy(), r0.kp2d_original[0].cpu().numpy()
    print(f"refit: kp2d_original {np.abs(got - want).max():.2e} px from the oracle optimum; without refit {np.abs(before - want).max():.2f} px")
    assert flags & ko.CONVERGED and np.abs(got - want).max() < 0.01
    assert np.abs(before - want).max() > 0.01
    res = trk.refit_result
    assert res is not None and r2.pose is res.q and r2.rot is res.rot and r2.trans is res.trans and r2.kp3d is res.kp3d
    assert r2.rot.shape == (1, 6) and int(res.status[0, 0]) & ko.CONVERGED


def test_tracker_fixed_camera_recovers_the_planted_joints(fixture_results):
    from hrpe_amd.lib.core.tracker import PoseTracker
    cases, _ = fixture_results
    case, ref = cases["panda_qonly"]
    panda = robot_of("panda")
    out, X = tracker_scene(case, ref["p_star"], 0)
    cTr = np.concatenate([case["rot0"], case["trans0"]])
    trk = PoseTracker(stub_model(out), panda, case["K"], (H, W), refit=kinfit.KinematicRefit(panda, "fixed_camera", cTr=cTr))
    r = trk.step(torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    obs = kinfit.observable_joints(panda)
    q = r.pose[0].cpu().numpy().astype(np.float64)
    print(f"fixed camera: max |q - q*| {np.abs(q[obs] - ref['p_star']).max():.2e}")
    assert np.abs(q[obs] - ref["p_star"]).max() <= 1e-5
    assert q[~obs].astype(np.float32).tobytes() == case["q0"][~obs].tobytes()
    assert r.rot.shape == (1, 3) and r.rot[0].cpu().numpy().tobytes() == case["rot0"].tobytes()
    want = ko.project(case["K"], X.astype(np.float64))
    assert np.abs(r.kp2d_original[0].cpu().numpy() - want).max() < 0.01
