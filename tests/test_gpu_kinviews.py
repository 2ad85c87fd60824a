"""GPU tests of the multi-view kinematic refit (hrp_kin_solve_views through kinfit.kin_solve_views, MultiViewRefit and the tracker hook)
against tests/kinviews_oracle.py, the float64 numpy statement of include/hrp.h, and the optima of tests/golden/golden_kinviews.npz.
Every launch has B <= 8, V <= 8 and nkp <= 24."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import hrpe_amd  # noqa: F401
import kinfit_oracle as ko
import kinviews_oracle as kv
from hrpe_amd import _native as nv
from hrpe_amd.lib.utils import kinfit
from hrpe_amd.lib.utils.urdf_robot import URDFRobot

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_ROBOTS = {}


def robot_of(name):
    if name not in _ROBOTS:
        _ROBOTS[name] = URDFRobot(name)
    return _ROBOTS[name]


class ChainRobot:
    """What kin_solve_views reads of a robot, around a bare chain."""
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


def solve(case, robot=None, B=1, shared=True, **over):
    """kin_solve_views on B copies of a case, K and the poses shared over the batch or per sample."""
    robot = robot or (robot_of(case["robot"]) if case.get("robot") else ChainRobot(case["chain"]))
    kw = dict(free_joints=np.asarray(case["free"], bool), w2d=None if case.get("w2d") is None else dev(case["w2d"], B),
              prior_q=case.get("prior"), limits=False if case.get("lo") is None else (case["lo"], case["hi"]))
    kw.update(over)
    nb = None if shared else B
    return kinfit.kin_solve_views(robot, dev(case["pts2d"], B), dev(case["K"], nb), dev(case["poses"], nb), dev(case["q0"], B), **kw)


def host(res, b=0):
    return {k: getattr(res, k)[b].cpu().numpy() for k in res._fields if getattr(res, k) is not None}


def same_bytes(a, b):
    return all(torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)) for k in a._fields)


@pytest.fixture(scope="module")
def fixture_results():
    cases, _ = kv.load_fixture(os.path.join(GOLDEN, "golden_kinviews.npz"), lambda n: robot_of(n).chain)
    res = {name: solve(case) for name, (case, _) in cases.items()}
    torch.cuda.synchronize()
    return cases, {name: host(r) for name, r in res.items()}


def test_every_fixture_case(fixture_results):
    """|q_dev - q*| <= 1e-5 per component, the planted flags, rows and npar exact, rms and rms_view within 1e-4 px of the oracle's at p*."""
    cases, got = fixture_results
    assert len(cases) == 27
    worst = 0.0
    for name, (case, ref) in cases.items():
        P, r = kv.Problem(case), got[name]
        d = np.abs(r["q"].astype(np.float64)[P.idx] - ref["p_star"])
        worst = max(worst, d.max())
        print(f"{name}: max |q - q*| {d.max():.2e}, LM trials {r['status'][1]} (oracle {ref['trials']}), rms {r['rms']:.6f} vs {ref['rms']:.6f}, "
              f"rms_view {np.abs(r['rms_view'] - ref['rms_view']).max():.1e}")
        assert d.max() <= 1e-5, (name, d)
        assert r["status"][0] == ref["flags"] and r["status"][2] == P.rows and r["status"][3] == P.npar, (name, r["status"])
        assert abs(float(r["rms"]) - ref["rms"]) <= 1e-4 and np.abs(r["rms_view"] - ref["rms_view"]).max() <= 1e-4, name
        assert r["used_view"].tolist() == P.used_view.tolist(), name
        fixed = ~P.free
        assert r["q"][fixed].tobytes() == np.asarray(case["q0"], np.float32)[fixed].tobytes(), name
        uv, X = P.reprojection(r["q"].astype(np.float64)[P.idx])
        assert r["kp3d"].shape == (P.V, P.nkp, 3) and np.abs(r["kp3d"] - X).max() < 1e-5 and np.abs(r["kp2d"] - uv).max() < 1e-2, name
    print(f"largest |q - q*| over the fixture: {worst:.2e}")


def test_covariance(fixture_results):
    """cov against numpy's s^2 inv(J^T J) from a complex-step Jacobian at the RETURNED (fp32) joints, the deviation relative to
    sqrt(cov_ii cov_jj), gated per case at ten times the stored deviation of the oracle alone (numpy at p* rounded to fp32 against
    numpy at p*).  All zeros on ``limit``."""
    cases, got = fixture_results
    for name, (case, ref) in cases.items():
        P, r = kv.Problem(case), got[name]
        if name.endswith("_limit"):
            assert not r["cov"].any(), name
            continue
        rel = lambda a, b: float((np.abs(a - b) / np.sqrt(np.outer(np.diag(b), np.diag(b)))).max())      # noqa: E731
        d = rel(r["cov"].astype(np.float64), P.covariance(r["q"].astype(np.float64)[P.idx]))
        print(f"{name}: oracle alone {ref['cov_own']:.2e}, device {d:.2e}")
        assert d <= 10 * ref["cov_own"], (name, d, ref["cov_own"])
        assert np.abs(r["cov"] - r["cov"].T).max() <= 1e-6 * np.abs(r["cov"]).max(), name


def test_one_view_lands_on_the_single_view_fixture():
    """V = 1 on golden_kinfit.npz's fixed-pose cases, the pose passed as the single view: within 1e-5 of THAT fixture's optimum, which
    ties the new loop to hrp_kin_solve's."""
    cases = ko.load_fixture(os.path.join(GOLDEN, "golden_kinfit.npz"), lambda n: robot_of(n).chain)
    todo = {n: c for n, c in cases.items() if n.split("_", 1)[1] in ("qonly", "qonly_noise", "limit", "weights")}
    assert len(todo) == 12
    res = {}
    for name, (case, ref) in todo.items():
        assert not case["free_pose"] and case["root"] == 0 and case["rot0"].size == 3
        one = dict(chain=case["chain"], robot=case["robot"], pts2d=case["pts2d"][None], K=case["K"][None],
                   poses=np.concatenate([case["rot0"], case["trans0"]])[None], q0=case["q0"], free=case["free"], lo=case["lo"], hi=case["hi"],
                   w2d=None if case.get("w2d") is None else case["w2d"][None], prior=case.get("prior"))
        res[name] = solve(one)
    torch.cuda.synchronize()
    for name, (case, ref) in todo.items():
        r, idx = host(res[name]), np.flatnonzero(case["free"])
        d = np.abs(r["q"].astype(np.float64)[idx] - ref["p_star"])
        print(f"{name}: max |q - q*| {d.max():.2e}, flags {r['status'][0]} (fixture {ref['flags']})")
        assert d.max() <= 1e-5 and r["status"][0] == ref["flags"], (name, d)
        assert abs(float(r["rms"]) - ref["rms"]) <= 1e-4 and r["rms"] == r["rms_view"][0], name


def test_shared_and_per_sample_K_and_poses_give_the_same_bytes(fixture_results):
    cases, got = fixture_results
    for robot in kv.ROBOTS:
        case, _ = cases[f"{robot}_shared_vs_per_sample"]
        a, b = solve(case, B=3, shared=True), solve(case, B=3, shared=False)
        assert same_bytes(a, b), robot
        assert all(torch.equal(a.q[0], a.q[i]) for i in range(3))
        assert a.q[0].cpu().numpy().tobytes() == got[f"{robot}_shared_vs_per_sample"]["q"].tobytes()


def test_two_calls_and_a_graph_replay_return_the_same_bytes(fixture_results):
    cases, _ = fixture_results
    case, _ = cases["baxter_weights"]
    robot = robot_of("baxter")
    args = [dev(case["pts2d"], 4), dev(case["K"]), dev(case["poses"]), dev(case["q0"], 4)]
    kw = dict(free_joints=case["free"], w2d=dev(case["w2d"], 4), limits=(case["lo"], case["hi"]))
    a = kinfit.kin_solve_views(robot, *args, **kw)
    b = kinfit.kin_solve_views(robot, *args, **kw)
    torch.cuda.synchronize()
    assert same_bytes(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        kinfit.kin_solve_views(robot, *args, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = kinfit.kin_solve_views(robot, *args, **kw)
    for t in c:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bytes(a, c)


def test_every_sample_of_a_mixed_batch_has_the_bytes_of_its_own_run(fixture_results):
    """Converging, FEW_ROWS, BAD_START, AT_LIMIT and a dropped view in one launch: no sample sees its neighbours."""
    cases, _ = fixture_results
    good, _ = cases["panda_v2"]
    limit, _ = cases["panda_limit"]
    ones = np.ones((2, 7), np.float32)
    behind = good["poses"].copy()
    behind[1, 5] = -behind[1, 5]
    dropped = good["pts2d"].copy()
    dropped[1] = np.nan
    rows = [dict(good, w2d=ones), dict(good, w2d=0 * ones), dict(good, w2d=ones, poses=behind), dict(limit, w2d=ones),
            dict(good, w2d=ones, pts2d=dropped)]
    want = [kv.Problem(c).lm()[1] for c in rows]
    assert want[1:4] == [kv.FEW_ROWS, kv.BAD_START, kv.CONVERGED | kv.AT_LIMIT] and want[0] == kv.CONVERGED and not want[4] & (kv.FEW_ROWS | kv.BAD_START)
    stack = lambda k: torch.stack([dev(c[k]) for c in rows])      # noqa: E731
    panda = robot_of("panda")
    kw = dict(free_joints=good["free"], limits=(good["lo"], good["hi"]))
    batch = kinfit.kin_solve_views(panda, stack("pts2d"), stack("K"), stack("poses"), stack("q0"), w2d=stack("w2d"), **kw)
    single = [solve(c, shared=False) for c in rows]
    torch.cuda.synchronize()
    assert batch.status[:, 0].tolist() == want
    assert batch.used_view.tolist() == [[7, 7], [0, 0], [7, 7], [7, 7], [7, 0]]
    for b, one in enumerate(single):
        for k in batch._fields:
            assert torch.equal(getattr(batch, k)[b].view(torch.int32), getattr(one, k)[0].view(torch.int32)), (b, k)
    for b in (1, 2):          # nothing was solved: the start bit for bit, no covariance
        assert torch.equal(batch.q[b], stack("q0")[b]) and not batch.cov[b].any() and int(batch.status[b, 1]) == 0


def test_permuted_views(fixture_results):
    """The views in another order: both answers lie within 1e-5 of p*, so within 2e-5 of each other; rms_view and used_view follow
    the views (rms_view to the 1e-4 px of the rms gate, since the joints differ in their last bits)."""
    cases, got = fixture_results
    for name, order in (("kuka_occluded", [2, 0, 1]), ("baxter_v4", [3, 1, 0, 2]), ("panda_occluded_view", [2, 1, 0])):
        case, _ = cases[name]
        r = host(solve(kv.permuted(case, order)))
        torch.cuda.synchronize()
        a = got[name]
        print(f"{name}: max |q - q_permuted| {np.abs(r['q'] - a['q']).max():.2e}")
        assert np.abs(r["q"].astype(np.float64) - a["q"]).max() <= 2e-5 and r["status"][0] == a["status"][0] and r["status"][2] == a["status"][2]
        assert r["used_view"].tolist() == a["used_view"][order].tolist()
        assert np.abs(r["rms_view"] - a["rms_view"][order]).max() <= 1e-4 and abs(float(r["rms"] - a["rms"])) <= 1e-4
        assert np.abs(r["kp3d"] - a["kp3d"][order]).max() < 1e-4


def test_largest_problem_against_the_numpy_loop():
    """npar = 32 on a synthetic serial chain with 24 key-points seen by 8 cameras: every LDS array at its largest size, 61 KB in all,
    against the numpy restatement of the loop."""
    case, P = kv.synthetic_case(ko.serial_chain(nv.FkChain), 8)
    r = host(solve(case, B=2), 1)
    torch.cuda.synchronize()
    pl, flags, it = P.lm()
    d = np.abs(r["q"].astype(np.float64)[P.idx] - pl)
    print(f"npar {P.npar}, rows {P.rows}: device trials {r['status'][1]}, numpy trials {it}, max |q - q_numpy| {d.max():.2e}")
    assert list(r["status"][2:]) == [416, 32] and r["status"][0] == flags and flags & kv.CONVERGED
    assert d.max() <= 1e-5 and r["cov"].shape == (32, 32) and (np.diag(r["cov"]) > 0).all()
    assert r["used_view"].tolist() == [24] * 8 and np.abs(r["rms_view"] - P.rms_view(pl)).max() <= 1e-4


def test_want_cov_false_leaves_the_other_outputs(fixture_results):
    cases, _ = fixture_results
    case, _ = cases["kuka_v3"]
    a, b = solve(case), solve(case, want_cov=False)
    torch.cuda.synchronize()
    assert b.cov is None and all(torch.equal(getattr(a, k), getattr(b, k)) for k in a._fields if k != "cov")


# ---- the tracker hook -----------------------------------------------------------------------------------------------------------------------
H, W = 480, 640


def stub_model(out):
    return lambda reg, root, k_values, K: out


def two_camera_scene(case, p_true):
    """(tuple a stub model returns for two streams, true camera-frame key-points [2, nkp, 3]): the regressor's joints are the case's
    start on stream 0 and a point halfway to the truth on stream 1, kp3d_int is the truth as each camera sees it."""
    P = kv.Problem(case)
    X = np.float32(P.points(p_true))
    q0 = np.float32(case["q0"])
    q1 = q0.copy()
    q1[P.idx] = np.float32(q0[P.idx] + 0.5 * (p_true - q0[P.idx]))
    R = [ko.rodrigues(w[:3].astype(np.float64)) for w in case["poses"]]
    rot6 = np.float32([r[:2].ravel() for r in R])
    z = lambda *s: torch.zeros(2, *s, device=DEV)      # noqa: E731
    return (dev(np.stack([q0, q1])), dev(rot6), dev(case["poses"][:, 3:]), z(2), z(1), z(P.nkp, 3), dev(X), dev(X)), X


def test_tracker_two_streams_are_two_views_of_one_arm(fixture_results):
    from hrpe_amd.lib.core.tracker import PoseTracker
    cases, _ = fixture_results
    case, ref = cases["panda_v2"]
    panda = robot_of("panda")
    P = kv.Problem(case)
    out, X = two_camera_scene(case, ref["p_star"])
    frames = torch.zeros(2, H, W, 3, dtype=torch.uint8, device=DEV)
    refit = kinfit.MultiViewRefit(panda, case["poses"])
    with pytest.raises(nv.HrpError, match="views"):
        PoseTracker(stub_model(out), panda, case["K"], (H, W), streams=1, refit=refit)
    with pytest.raises(nv.HrpError, match="mutually exclusive"):
        PoseTracker(stub_model(out), panda, case["K"], (H, W), streams=2, refit=refit,
                    filter=kinfit.KinematicFilter(panda, "fixed_camera", 0.03, 1.0, 1.0, streams=2, cTr=case["poses"][0]))
    plain = PoseTracker(stub_model(out), panda, case["K"], (H, W), streams=2)
    none = PoseTracker(stub_model(out), panda, case["K"], (H, W), streams=2, refit=None)
    trk = PoseTracker(stub_model(out), panda, case["K"], (H, W), streams=2, refit=refit)
    r0, r1, r = plain.step(frames), none.step(frames), trk.step(frames)
    torch.cuda.synchronize()
    # refit=None: the model's tensors pass through and the bytes are those of a tracker built without the argument
    for a, b in zip(r0, r1):
        assert (a is None and b is None) or torch.equal(a, b)
    assert none.refit_result is None and torch.equal(plain.kp2d, none.kp2d) and r1.pose is out[0] and r1.rot is out[1] and r1.kp3d is out[-1]
    # the planted joints, by the fixed-camera test's gate
    q = r.pose.cpu().numpy().astype(np.float64)
    print(f"two views: max |q - q*| {np.abs(q[0][P.idx] - ref['p_star']).max():.2e}")
    assert np.abs(q[0][P.idx] - ref["p_star"]).max() <= 1e-5 and np.array_equal(q[0], q[1])
    mean = out[0].mean(0).cpu().numpy()
    assert q[0][~P.free].astype(np.float32).tobytes() == mean[~P.free].tobytes()
    # every stream carries its own calibrated pose, in the model's representation, and its own camera's key-points
    res = trk.refit_result
    assert res is not None and res.q.shape == (1, 8) and res.kp3d.shape == (1, 2, 7, 3) and int(res.status[0, 0]) & kv.CONVERGED
    assert r.rot.shape == (2, 6) and np.array_equal(r.rot.cpu().numpy(), np.float32(refit.rot6))
    assert np.array_equal(r.trans.cpu().numpy(), np.float32(refit.trans)) and torch.equal(r.kp3d, res.kp3d[0])
    uv, _ = P.reprojection(q[0][P.idx])
    got = r.kp2d_original.cpu().numpy()
    assert np.abs(got - uv).max() < 0.01 and np.abs(got[0] - got[1]).max() > 1.0
    assert np.abs(r.kp3d.cpu().numpy() - X).max() < 1e-4
