"""CPU-only checks of the kinematic refit (hrp_kin_solve): tests/kinfit_host_check.cpp runs csrc/kin_core.h's solve_one - the very loop
the kernel runs - one lane at a time, built with the host compiler and -fsanitize=address,undefined -fno-sanitize-recover as a plain
executable.  Every case of golden_kinfit.npz against its float64 optimum, hostile inputs, the flags and row counts, observable_joints
for the three robots, kin_solve's refusals (reached before any GPU call), the C ABI's refusals and the ctypes mirror."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import hrpe_amd  # noqa: F401
import kinfit_oracle as ko
from hrpe_amd import _native as nv
from hrpe_amd.lib.utils import kinfit
from hrpe_amd.lib.utils.urdf_robot import URDFRobot

_ROBOTS = {}


def robot_of(name):
    if name not in _ROBOTS:
        _ROBOTS[name] = URDFRobot(name)
    return _ROBOTS[name]


def load_cases():
    return ko.load_fixture(os.path.join(GOLDEN, "golden_kinfit.npz"), lambda n: robot_of(n).chain)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("kinfit_host")
    exe = str(td / "kinfit_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "kinfit_host_check.cpp"), "-o", exe], check=True)
    return exe, td


def run_cases(check_exe, cases, tag):
    exe, td = check_exe
    src, dst = str(td / f"{tag}.in"), str(td / f"{tag}.out")
    ko.write_cases(src, cases)
    r = subprocess.run([exe, "run", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return ko.unpack_results(open(dst, "rb").read(), cases)


@pytest.fixture(scope="module")
def fixture_results(check_exe):
    cases = load_cases()
    return cases, dict(zip(cases, run_cases(check_exe, [c for c, _ in cases.values()], "fixture")))


def test_fixture_is_small_and_complete():
    cases = load_cases()
    assert os.path.getsize(os.path.join(GOLDEN, "golden_kinfit.npz")) < 32 * 1024
    kinds = ["qonly", "qonly_noise", "both_prior", "both_q1fixed", "with3d", "limit", "weights"]
    assert list(cases) == [f"{r}_{k}" for r in ("panda", "kuka", "baxter") for k in kinds + (["root3"] if r == "panda" else [])]
    for name, (case, ref) in cases.items():
        P = ko.Problem(case)
        assert ref["maxJ"] < 1000 and ref["trials"] <= 100 and len(ref["p_star"]) == P.npar, name
        assert bool(ref["flags"] & ko.AT_LIMIT) == name.endswith("_limit") and ref["flags"] & ko.CONVERGED, name
        if name.endswith("_limit"):
            assert ((ref["p_star"] == P.plo) | (ref["p_star"] == P.phi)).sum() == 1, name
        if name.endswith("_weights"):
            assert (case["w2d"] == 0).sum() == 2 and np.isnan(case["pts2d"]).any(1).sum() == 1, name


def test_every_fixture_case_on_the_host(fixture_results):
    """The host run of the kernel's loop meets the GPU gate: |p - p*| <= 1e-5 per component, the planted flags, rms within 1e-4 px."""
    cases, got = fixture_results
    for name, (case, ref) in cases.items():
        P, r = ko.Problem(case), got[name]
        p = P.solution_vector(r["q"], r["rot"], r["trans"])
        d = np.abs(p - ref["p_star"])
        if P.free_pose:
            d[P.nfree:P.nfree + 3] = ko.rotvec_close(p[P.nfree:P.nfree + 3], ref["p_star"][P.nfree:P.nfree + 3])
        print(f"{name}: max |p - p*| {d.max():.2e}, trials {r['status'][1]} (oracle {ref['trials']}), rms {r['rms']:.6f} vs {ref['rms']:.6f}")
        assert d.max() <= 1e-5, (name, d)
        assert r["status"][0] == ref["flags"] and r["status"][2] == P.rows and r["status"][3] == P.npar, (name, r["status"])
        assert abs(float(r["rms"]) - ref["rms"]) <= 1e-4, name
        fixed = ~P.free
        assert np.array_equal(r["q"][fixed].view(np.int32), np.asarray(case["q0"], np.float32)[fixed].view(np.int32)), name
        if not P.free_pose:
            assert np.array_equal(r["rot"], case["rot0"]) and np.array_equal(r["trans"], case["trans0"]), name
        X = P.points(p)
        assert np.abs(r["xyz"] - X).max() < 1e-5 and np.abs(r["uv"] - ko.project(P.K, X)).max() < 1e-2, name
        if name.endswith("_limit"):
            assert not r["cov"].any(), name
        else:
            cov = P.covariance(ref["p_star"])
            s = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
            assert np.abs(r["cov"] - cov).max() <= 1e-3 * s.max() and (np.abs(r["cov"] - cov) / s).max() < 1e-3, name


def test_rows_and_few_rows(check_exe):
    """rows == npar solves (cov zero); rows == npar - 1 is FEW_ROWS and returns the start bit for bit."""
    case, _ = load_cases()["panda_both_q1fixed"]          # npar 11
    w = np.zeros(7, np.float32)
    w[:5] = 1.0
    exact = dict(case, w2d=w, prior=np.float32([0, 1, 0, 0, 0, 0, 0, 0]))          # 10 + 1 rows
    short = dict(case, w2d=w)                                                      # 10 rows
    a, b = run_cases(check_exe, [exact, short], "rows")
    assert list(a["status"][2:]) == [11, 11] and not a["status"][0] & ko.FEW_ROWS and not a["cov"].any()
    assert a["status"][1] > 0
    assert list(b["status"]) == [ko.FEW_ROWS, 0, 10, 11] and not b["cov"].any()
    for k, k0 in (("q", "q0"), ("rot", "rot0"), ("trans", "trans0")):
        assert b[k].tobytes() == np.asarray(case[k0], np.float32).tobytes(), k


def test_synthetic_chain_at_the_largest_size(check_exe):
    """npar = 38 on a 32-joint serial chain with 24 key-points: the host run against the numpy restatement of the loop."""
    ch = ko.serial_chain(nv.FkChain)
    case, P, p_true = synthetic_case(ch)
    r, = run_cases(check_exe, [case], "serial")
    pl, flags, it = P.lm()
    p = P.solution_vector(r["q"], r["rot"], r["trans"])
    print(f"npar {P.npar} rows {P.rows}: host trials {r['status'][1]}, numpy trials {it}, max |p - p_numpy| {np.abs(p - pl).max():.2e}")
    assert list(r["status"][2:]) == [P.rows, 38] and r["status"][0] == flags
    assert np.abs(p - pl).max() <= 1e-5


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
    return case, ko.Problem(case), np.concatenate([q, pose])


def test_hostile_inputs(check_exe):
    exe, _ = check_exe
    r = subprocess.run([exe, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "failures 0", r.stdout
    got = {ln.split(":")[0][8:]: ln.split(":")[1].split() for ln in r.stdout.splitlines() if ln.startswith("hostile ")}
    field = lambda name, key: int(got[name][got[name].index(key) + 1])      # noqa: E731
    assert field("all weights 0", "flags") == ko.FEW_ROWS and field("all weights 0", "start") == 1
    assert field("NaN everywhere", "flags") & ko.FEW_ROWS and field("NaN everywhere", "start") == 1 and field("NaN everywhere", "cov0") == 1
    assert field("NaN points and q0, weights 1", "flags") == ko.FEW_ROWS | ko.BAD_START
    assert field("nothing free", "flags") == ko.FEW_ROWS and field("nothing free", "npar") == 0 and field("nothing free", "rows") == 14
    assert field("start behind the camera", "flags") == ko.BAD_START and field("start behind the camera", "start") == 1
    assert field("start behind the camera", "trials") == 0
    assert field("lo > hi", "flags") & ko.AT_LIMIT and field("lo > hi", "cov0") == 1
    assert field("dof 32 nkp 24 with 3-D targets", "npar") == 38 and field("dof 32 nkp 24 with 3-D targets", "rows") == 152
    assert field("dof 32 nkp 24 rot_dim 6 root 23", "npar") == 38
    assert field("dof 0", "npar") == 6 and "broken chain table" in got


def test_observable_joints_of_the_three_robots():
    assert kinfit.observable_joints(robot_of("panda")).tolist() == [True] * 6 + [False, False]
    assert kinfit.observable_joints(robot_of("kuka")).tolist() == [True] * 6 + [False]
    names = ["head_pan"] + [f"{s}_{j}" for j in ("s0", "s1", "e0", "e1", "w0", "w1", "w2") for s in ("right", "left")]
    assert kinfit.observable_joints(robot_of("baxter")).tolist() == [n not in ("head_pan", "right_w2", "left_w2") for n in names]
    # joint 1 of panda and kuka turns about the base z axis through key-point 0: a gauge of the free pose; baxter has none
    assert kinfit.gauge_joints(robot_of("panda")).tolist() == [True] + [False] * 7
    assert kinfit.gauge_joints(robot_of("kuka")).tolist() == [True] + [False] * 6
    assert not kinfit.gauge_joints(robot_of("baxter")).any()


def test_kin_solve_refuses_before_any_gpu_call():
    import torch
    panda = robot_of("panda")
    x, K, q, r, t = torch.zeros(1, 7, 2), torch.eye(3), torch.zeros(1, 8), torch.zeros(1, 3), torch.zeros(1, 3)
    free = np.array([False, True, True, True, True, True, True, False])
    with pytest.raises(nv.HrpError, match=r"joint 6 \(panda_joint7\).*unobservable"):
        kinfit.kin_solve(panda, x, K, q, r, t, free_joints=free, free_pose=False)
    with pytest.raises(nv.HrpError, match=r"joint 0 \(panda_joint1\).*gauge"):
        kinfit.kin_solve(panda, x, K, q, r, t, free_joints=[0, 1, 2], free_pose=True)
    with pytest.raises(nv.HrpError, match="gauge"):
        kinfit.kin_solve(panda, x, K, q, r, t, free_joints=[0, 1], free_pose=True, prior_q=[0, 1, 1, 1, 1, 1, 1, 1])
    # with a prior, or the pose fixed, the same requests pass the host checks and stop at the CPU tensors
    for kw in (dict(free_joints=free, free_pose=False, prior_q=1.0), dict(free_joints=[0, 1, 2], free_pose=True, prior_q=1.0),
               dict(free_joints=[0, 1, 2], free_pose=False), dict()):
        with pytest.raises(nv.HrpError, match="no CPU path"):
            kinfit.kin_solve(panda, x, K, q, r, t, **kw)
    for kw, what in ((dict(prior_q=-1.0), "prior_q"), (dict(prior_q=[1.0] * 3), "prior_q"), (dict(root=7), "root"),
                     (dict(free_joints=[8]), "free_joints"), (dict(pts3d=x), "pts3d and w3d")):
        with pytest.raises(nv.HrpError, match=what):
            kinfit.kin_solve(panda, x, K, q, r, t, **kw)
    free, prior = kinfit.resolve_free(panda, None, True, None)
    assert free.tolist() == [False] + [True] * 5 + [False, False] and prior is None           # the gauge joint is left out
    assert kinfit.resolve_free(panda, None, True, 2.0)[0].tolist() == [True] * 6 + [False, False]
    assert kinfit.resolve_free(panda, None, False, None)[0].tolist() == [True] * 6 + [False, False]


def test_refit_holder_and_tracker_surface():
    from hrpe_amd.lib.core.tracker import PoseTracker, TrackResult
    panda = robot_of("panda")
    with pytest.raises(nv.HrpError, match="prior_q"):
        kinfit.KinematicRefit(panda, "holistic")
    with pytest.raises(nv.HrpError, match="cTr"):
        kinfit.KinematicRefit(panda, "fixed_camera")
    with pytest.raises(nv.HrpError, match="mode"):
        kinfit.KinematicRefit(panda, "robust", prior_q=1.0)
    h = kinfit.KinematicRefit(panda, "holistic", prior_q=4.0)
    assert h.free_pose and h.root == 3 and h.free.tolist() == [True] * 6 + [False, False] and (h.prior_q == 4.0).all()
    f = kinfit.KinematicRefit(panda, "fixed_camera", cTr=np.array([1.2, -1.0, 0.8, 0.05, -0.1, 1.5]))
    assert not f.free_pose and f.root == 0 and f.prior_q is None and f.free.tolist() == [True] * 6 + [False, False]
    assert "tuned" in kinfit.KinematicRefit.__doc__ and "px^2 per rad^2" in kinfit.KinematicRefit.__doc__
    p = inspect.signature(kinfit.kin_solve).parameters
    assert list(p) == ["robot", "pts2d", "K", "q0", "rot0", "trans0", "free_joints", "free_pose", "root", "w2d", "pts3d", "w3d", "prior_q",
                       "limits"]
    assert [p[k].default for k in list(p)[6:]] == [None, True, 0, None, None, None, None, True]
    assert kinfit.KinResult._fields == ("q", "rot", "trans", "kp3d", "kp2d", "rms", "status", "cov")
    p = inspect.signature(PoseTracker.__init__).parameters
    assert list(p)[-1] == "refit" and p["refit"].default is None
    assert TrackResult._fields == ("pose", "rot", "trans", "kp3d", "kp2d_original", "depth", "status", "k_values")


def test_kin_abi_declared_bound_and_refusing():
    src = open(os.path.join(ROOT, "include", "hrp.h")).read()
    assert re.search(r"\bint\s+hrp_kin_solve\s*\(\s*const hrp_kin_desc\*", src) and len(nv.PROTOTYPES["hrp_kin_solve"]) == 2
    assert re.search(r"HRP_KIN_CONVERGED = 1, HRP_KIN_AT_LIMIT = 2, HRP_KIN_FEW_ROWS = 4, HRP_KIN_BAD_START = 8", src)
    assert (nv.KIN_CONVERGED, nv.KIN_AT_LIMIT, nv.KIN_FEW_ROWS, nv.KIN_BAD_START) == (1, 2, 4, 8)
    assert re.search(r"#define HRP_KIN_MAX_IT 200\b", src) and nv.KIN_MAX_IT == 200 == ko.MAX_IT
    prog = '#include <stdio.h>\n#include "hrp.h"\nint main(void) { printf("%zu\\n", sizeof(hrp_kin_desc)); return 0; }\n'
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")], check=True)
        size = int(subprocess.run([os.path.join(td, "s")], check=True, stdout=subprocess.PIPE, text=True).stdout)
    assert size == ctypes.sizeof(nv.KinDesc)
    lib = nv.lib()

    def solve(**kw):
        d = nv.KinDesc()
        for k in ("chain", "pts2d", "K", "q0", "rot0", "trans0", "q", "rot", "trans"):
            setattr(d, k, 64)
        d.nkp, d.dof, d.rot_dim, d.pose_stride, d.K_stride, d.free_q, d.free_pose, d.root, d.B = 7, 8, 3, 1, 9, 0x3f, 1, 0, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.hrp_kin_solve(ctypes.byref(d), None)
    assert lib.hrp_kin_solve(None, None) == -1 and b"kin_solve" in lib.hrp_last_error()
    for bad in (dict(chain=None), dict(pts2d=None), dict(K=None), dict(q0=None), dict(rot0=None), dict(trans0=None), dict(q=None),
                dict(rot=None), dict(trans=None), dict(rot_dim=4), dict(rot_dim=0), dict(free_q=1 << 8), dict(free_q=1 << 31), dict(pts3d=64),
                dict(w3d=64), dict(B=0), dict(B=-3), dict(nkp=0), dict(nkp=25), dict(dof=33), dict(K_stride=3), dict(pose_stride=2),
                dict(free_pose=2), dict(root=7), dict(root=-1)):
        assert solve(**bad) == -1, bad
        assert b"kin_solve" in lib.hrp_last_error(), (bad, lib.hrp_last_error())
