"""CPU-only checks of the kinematic filter (hrp_kin_filter_step): tests/kinfilter_host_check.cpp runs csrc/kin_filter_core.h's step_one -
the very loop the kernel runs - one lane at a time, built with the host compiler and -fsanitize=address,undefined
-fno-sanitize-recover as a plain executable with exact-size buffers.  Every frame of golden_kinfilter.npz teacher-forced from the
oracle's previous state, free runs from INIT, hostile inputs, the rotation's wrap, KinematicFilter's refusals (reached before any GPU
call), the C ABI's refusals, the ctypes mirror and the tracker's argument surface."""
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
import kinfilter_oracle as kf
import kinfit_oracle as ko
from hrpe_amd import _native as nv
from hrpe_amd.lib.utils import kinfit
from hrpe_amd.lib.utils.urdf_robot import URDFRobot

_ROBOTS = {}
FIXTURE = os.path.join(GOLDEN, "golden_kinfilter.npz")


def robot_of(name):
    if name not in _ROBOTS:
        _ROBOTS[name] = URDFRobot(name)
    return _ROBOTS[name]


@pytest.fixture(scope="module")
def sequences():
    """{name: (seq, [(state, out)] of the oracle per frame)}, rebuilt once from the stored p+."""
    seqs = kf.load_fixture(FIXTURE, lambda n: robot_of(n).chain)
    return {name: (seq, kf.replay(seq)) for name, seq in seqs.items()}


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("kinfilter_host")
    exe = str(td / "kinfilter_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "kinfilter_host_check.cpp"), "-o", exe], check=True)
    return exe, td


def run_steps(check_exe, steps, items, tag):
    exe, td = check_exe
    src, dst = str(td / f"{tag}.in"), str(td / f"{tag}.out")
    kf.write_steps(src, steps)
    r = subprocess.run([exe, "run", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return kf.unpack_steps(open(dst, "rb").read(), items)


def test_fixture_is_small_and_complete(sequences):
    assert os.path.getsize(FIXTURE) < 64 * 1024
    assert list(sequences) == kf.sequence_names() and len(sequences) == 19
    for name, (seq, res) in sequences.items():
        F, kind = seq["filter"], name.split("_", 1)[1]
        assert len(seq["frames"]) == 12 and abs(F.dt - 1 / 30) < 1e-12 and F.gate == 40.0, name
        flags = [int(o["flags"]) for _, o in res]
        assert flags == [int(f) for f in seq["flags"]], name          # the replay from the stored p+ takes the generator's decisions
        assert [o["used"] for _, o in res] == list(seq["used"]) and [o["gated"] for _, o in res] == list(seq["gated"]), name
        # the stored p+ is a stationary point of the oracle's cost (the joints on a bound aside)
        for (_, o), f in zip(res, flags):
            if "grad" in o and not f & kf.AT_LIMIT:
                assert np.abs(o["grad"]).max() < 1e-8, name
        d2 = np.concatenate([o["d2"][np.isfinite(o["d2"])] for _, o in res])
        assert not ((d2 >= F.gate / 2) & (d2 <= 2 * F.gate)).any(), name                      # (a) the gate's margin
        if kind == "smooth":
            assert seq["cmp"][0] < seq["cmp"][1], name                                         # (d) as the generator recorded it
        if kind == "outlier":
            assert 5 * seq["cmp"][2] <= seq["cmp"][3] and seq["gated"][7] == 1 and sum(seq["gated"]) == 1, name
        if kind == "dropout":
            assert flags[6] == kf.COASTED and any(np.isnan(fr["pts2d"]).any() for fr in seq["frames"]), name
        if kind == "limit":
            assert all(f & kf.AT_LIMIT for f in flags[7:]), name
        if kind == "holistic":
            assert F.P.free_pose and F.P.root == 3 and F.has_wq and F.n == 12, name
        if kind == "restart":
            assert flags[6] & kf.INIT and seq["frames"][6]["keep"] == 0, name
        if kind == "lost":
            assert flags[6] == kf.COASTED | kf.LOST and flags[7] & kf.INIT and F.max_coast == 2, name


def test_every_fixture_frame_teacher_forced_on_the_host(check_exe, sequences):
    """Every frame stepped from the oracle's previous state: kinfilter_oracle.check_step's gates."""
    worst = np.zeros(4)
    for name, (seq, res) in sequences.items():
        F, chain = seq["filter"], robot_of(seq["robot"]).chain
        prev = [kf.empty_state(F.n)] + [s for s, _ in res[:-1]]
        got = run_steps(check_exe, [kf.pack_step(F, chain, p, fr) for p, fr in zip(prev, seq["frames"])], [(F, 3)] * 12, name)
        fig = np.max([kf.check_step(f"{name}[{t}]", F, fr, g, s, o, seq["own"][:3])
                      for t, (fr, g, (s, o)) in enumerate(zip(seq["frames"], got, res))], 0)
        print(f"{name}: fp32 |p - p+| {fig[0]:.1e}; fp64 p {fig[1]:.1e} v {fig[2]:.1e} cov {fig[3]:.1e} (oracle alone "
              f"{' '.join(f'{v:.1e}' for v in seq['own'][:3])}); trials {[int(g['status'][1]) for g in got]}")
        worst = np.maximum(worst, fig)
    print("largest:", worst)


def test_free_runs_on_the_host(check_exe, sequences):
    """12 frames from INIT, every step from the state the program itself left, against the oracle's free run."""
    for name, (seq, res) in sequences.items():
        F, chain = seq["filter"], robot_of(seq["robot"]).chain
        steps = [kf.pack_step(F, chain, kf.empty_state(F.n), fr, chained=t > 0) for t, fr in enumerate(seq["frames"])]
        got = run_steps(check_exe, steps, [(F, 3)] * 12, name + "_free")
        fig = np.max([kf.check_step(f"{name}[{t}]", F, fr, g, s, o, seq["own"][3:])
                      for t, (fr, g, (s, o)) in enumerate(zip(seq["frames"], got, res))], 0)
        print(f"{name}: free run fp64 p {fig[1]:.1e} v {fig[2]:.1e} cov {fig[3]:.1e} (oracle alone {' '.join(f'{v:.1e}' for v in seq['own'][3:])})")


def test_rotation_wrap_on_the_host(check_exe):
    """A pose-only stream (a chain of fixed points) whose rotation the loop leaves beyond pi: the state is wrapped, the rotational
    rates are set to 0 and their covariance to p0_var's, REWRAPPED; the same frame below pi is not touched."""
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.2, 0.2, (6, 3))
    ch = ko.point_chain(nv.FkChain, pts)
    K = np.float32([[600, 0, 320], [0, 600, 240], [0, 0, 1]])
    p0 = np.r_[np.full(3, 0.01), np.full(3, 0.0025), np.full(3, 1.0), np.full(3, 0.25)]
    F = kf.Filter(ch, np.zeros(0, bool), True, 0, K, 1 / 30, np.r_[np.full(3, 10.0), np.full(3, 2.0)], p0, 40.0)
    for th, wrapped in ((3.2, True), (3.0, False)):
        w = np.float32(np.array([0.6, 0.0, 0.8]) * th)
        t = np.float32([0.05, -0.1, 1.5])
        X = ko.keypoints(ko.tables(ch), np.zeros(0), ko.rodrigues(w.astype(np.float64)), t.astype(np.float64))
        frames = []
        for i in range(2):
            frames.append(dict(pts2d=np.float32(ko.project(K, X) + 0.3 * rng.standard_normal((6, 2))), w2d=None, q_in=np.zeros(0, np.float32),
                               rot_in=w, trans_in=t, q_meas=None, keep=1))
        st, ref = kf.empty_state(6), []
        for fr in frames:
            st, out = F.step(st, fr)
            ref.append((st, out))
        got = run_steps(check_exe, [kf.pack_step(F, ch, kf.empty_state(6), fr, chained=i > 0) for i, fr in enumerate(frames)], [(F, 3)] * 2, "wrap")
        for i, (g, (s, o)) in enumerate(zip(got, ref)):
            # the first frame starts beyond pi and is wrapped; the second then runs from the wrapped state, below pi
            assert bool(o["flags"] & kf.REWRAPPED) == (wrapped and i == 0) and int(g["status"][0]) == o["flags"], (th, i, g["status"], o["flags"])
            assert np.abs(g["mean"] - s["mean"]).max() < 1e-9 and kf.rel_cov(g["cov"], s["cov"]) < 1e-8, (th, i)
            assert np.linalg.norm(g["mean"][:3]) <= np.pi and np.linalg.norm(g["rot"]) <= np.pi + 1e-6
            if wrapped and i == 0:
                assert not g["mean"][6:9].any() and np.array_equal(np.diag(g["cov"])[6:9], p0[6:9])
                off = g["cov"][6:9].copy()
                off[np.arange(3), np.arange(6, 9)] = 0
                assert not off.any() and not g["cov"][:, 6:9][np.r_[0:6, 9:12]].any()
                assert ko.rotvec_close(g["rot"].astype(np.float64), w.astype(np.float64)) < 1e-2


def test_hostile_inputs(check_exe):
    exe, _ = check_exe
    r = subprocess.run([exe, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "failures 0", r.stdout
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("hostile "):
            got.setdefault(ln.split(":")[0][8:], []).append(ln.split(":", 1)[1].split())
    field = lambda name, key, i=0: int(got[name][i][got[name][i].index(key) + 1])      # noqa: E731
    assert field("plain", "flags") == kf.CONVERGED and field("plain", "used") == 7 and field("plain", "valid") == 1
    assert field("NaN points", "flags") == kf.COASTED and field("NaN points", "coast") == 1 and field("NaN points", "finite") == 1
    assert field("NaN everywhere", "flags") == kf.INIT | kf.BAD_START and field("NaN everywhere", "valid") == 0
    assert field("NaN everywhere", "inputs") == 1 and field("NaN everywhere", "state_kept") == 1
    assert field("NaN state, good inputs", "flags") == kf.INIT | kf.CONVERGED and field("NaN state, good inputs", "finite") == 1
    assert field("zero row and column in cov", "flags") == kf.CONVERGED and field("zero row and column in cov", "finite") == 1
    assert field("zero pivot in the prediction", "flags") == kf.INIT | kf.CONVERGED
    assert field("zero cov and zero p0_var", "flags") == kf.INIT | kf.BAD_START and field("zero cov and zero p0_var", "valid") == 0
    assert field("all points gated", "flags") == kf.COASTED and field("all points gated", "gated") == 7 and field("all points gated", "used") == 0
    assert field("all points gated", "coast") == 1 and field("all points gated", "valid") == 1
    assert field("all points gated, coast at max_coast", "flags") == kf.COASTED | kf.LOST
    assert field("all points gated, coast at max_coast", "valid") == 0 and field("all points gated, coast at max_coast", "coast") == 6
    assert field("coast at INT_MAX", "coast") == 2 ** 31 - 1
    assert field("start behind the camera", "flags") == kf.INIT | kf.BAD_START and field("start behind the camera", "inputs") == 1
    assert len(got["dt refused"]) == 4 and all(field("dt refused", "refused", i) == 1 for i in range(4))
    assert field("dt denormal", "refused") == 0 and field("dt denormal", "flags") == kf.CONVERGED and field("dt denormal", "finite") == 1
    assert field("dt huge", "flags") & kf.INIT and field("dt huge", "finite") == 1
    assert field("max_coast -1", "refused") == 1 and field("n 21", "refused") == 1 and field("n 0", "refused") == 1
    assert field("n 1", "flags") == kf.CONVERGED and field("n 20 nkp 24", "flags") == kf.CONVERGED and field("n 20 nkp 24", "used") == 24
    assert field("n 20 rot_dim 6 root 23 start", "flags") == kf.INIT | kf.CONVERGED
    assert field("dof 0", "flags") == kf.CONVERGED and "broken chain table" in got and "lo > hi" in got
    for name, rows in got.items():
        for i in range(len(rows)):
            if field(name, "refused", i) == 0:
                assert field(name, "symmetric", i) == 1, name


def test_filter_refuses_before_any_gpu_call():
    import torch
    panda = robot_of("panda")
    kw = dict(dt=1 / 30, q_acc=10.0, p0_var=0.01)
    cTr = np.array([1.2, -1.0, 0.8, 0.05, -0.1, 1.5])
    for bad, what in ((dict(mode="robust"), "mode"), (dict(mode="fixed_camera"), "cTr"), (dict(mode="holistic", cTr=cTr), "cTr"),
                      (dict(dt=0.0), "dt"), (dict(dt=float("nan")), "dt"), (dict(dt=-1.0), "dt"), (dict(q_acc=None), "q_acc"),
                      (dict(q_acc=-1.0), "q_acc"), (dict(p0_var=None), "p0_var"), (dict(p0_var=0.0), "p0_var"), (dict(p0_var=[1.0] * 3), "p0_var"),
                      (dict(gate_chi2=0.0), "gate_chi2"), (dict(gate_chi2=float("nan")), "gate_chi2"), (dict(max_coast=-1), "max_coast"),
                      (dict(w_q=-1.0), "prior_q"), (dict(streams=0), "streams"), (dict(free_joints=[8]), "free_joints")):
        args = dict(dict(mode="holistic"), **kw)
        args.update(bad)
        with pytest.raises(nv.HrpError, match=what):
            kinfit.KinematicFilter(panda, **args)
    with pytest.raises(nv.HrpError, match=r"joint 6 \(panda_joint7\).*unobservable"):
        kinfit.KinematicFilter(panda, "fixed_camera", cTr=cTr, free_joints=[5, 6], **kw)
    baxter = robot_of("baxter")
    with pytest.raises(nv.HrpError, match="parameters"):          # 15 joints with a measurement on each, and the pose: n = 21
        kinfit.KinematicFilter(baxter, "holistic", free_joints=np.ones(15, bool), w_q=1.0, **kw)
    assert kinfit.KinematicFilter(baxter, "holistic", **kw).n == 18 == nv.KIN_FILTER_MAX_N - 2
    # a gauge joint needs no prior: the state prior regularises it
    h = kinfit.KinematicFilter(panda, "holistic", gate_chi2=40.0, w_q=50.0, streams=2, **kw)
    assert h.free.tolist() == [True] * 6 + [False, False] and h.n == 12 and h.root == 3 and h.free_pose and h.B == 2 and h.gate_chi2 == 40.0
    f = kinfit.KinematicFilter(panda, "fixed_camera", cTr=cTr, **kw)
    assert f.n == 6 and f.root == 0 and f.w_q is None and f.gate_chi2 == 0.0 and f.max_coast == 5 and f.mean is None
    f.reset()
    x, K, q, r, t = torch.zeros(1, 7, 2), torch.eye(3), torch.zeros(1, 8), torch.zeros(1, 3), torch.zeros(1, 3)
    with pytest.raises(nv.HrpError, match="no CPU path"):
        f.step(x, K, q)
    with pytest.raises(nv.HrpError, match="cTr"):
        f.step(x, K, q, r, t)
    with pytest.raises(nv.HrpError, match="dt"):
        f.step(x, K, q, dt=0.0)
    with pytest.raises(nv.HrpError, match="rot and trans"):
        h.step(torch.zeros(2, 7, 2), K, torch.zeros(2, 8))
    assert f.mean is None and h.mean is None                  # nothing was created on a device
    assert "tuned" in kinfit.KinematicFilter.__doc__ and "|w| = pi" in kinfit.KinematicFilter.__doc__
    p = inspect.signature(kinfit.KinematicFilter.__init__).parameters
    assert list(p) == ["self", "robot", "mode", "dt", "q_acc", "p0_var", "streams", "cTr", "free_joints", "limits", "gate_chi2", "max_coast", "w_q",
                       "reference_keypoint_id"]
    assert [p[k].default for k in list(p)[6:]] == [1, None, None, True, None, 5, None, 3]
    p = inspect.signature(kinfit.KinematicFilter.step).parameters
    assert list(p) == ["self", "pts2d", "K", "pose", "rot", "trans", "w2d", "q_meas", "keep", "dt"]
    assert kinfit.KinFilterResult._fields == ("q", "rot", "trans", "kp3d", "kp2d", "vel", "cov", "kp3d_next", "status", "d2")


def test_tracker_surface():
    from hrpe_amd.lib.core.tracker import PoseTracker
    p = inspect.signature(PoseTracker.__init__).parameters
    assert p["filter"].default is None and p["crop_from_prediction"].default is False and p["refit"].default is None
    panda = robot_of("panda")
    flt = kinfit.KinematicFilter(panda, "holistic", 1 / 30, 10.0, 0.01)
    refit = kinfit.KinematicRefit(panda, "holistic", prior_q=1.0)
    model, K = (lambda *a: None), np.eye(3)
    with pytest.raises(nv.HrpError, match="mutually exclusive"):
        PoseTracker(model, panda, K, (480, 640), filter=flt, refit=refit)
    with pytest.raises(nv.HrpError, match="crop_from_prediction"):
        PoseTracker(model, panda, K, (480, 640), crop_from_prediction=True)
    with pytest.raises(nv.HrpError, match="KinematicFilter"):
        PoseTracker(model, panda, K, (480, 640), filter=refit)
    with pytest.raises(nv.HrpError, match="streams"):
        PoseTracker(model, panda, K, (480, 640), streams=2, filter=flt)


def test_filter_abi_declared_bound_and_refusing():
    src = open(os.path.join(ROOT, "include", "hrp.h")).read()
    assert re.search(r"\bint\s+hrp_kin_filter_step\s*\(\s*const hrp_kin_filter_desc\*", src) and len(nv.PROTOTYPES["hrp_kin_filter_step"]) == 2
    assert re.search(r"HRP_KF_INIT = 1, HRP_KF_COASTED = 2, HRP_KF_LOST = 4, HRP_KF_BAD_START = 8, HRP_KF_REWRAPPED = 16, HRP_KF_CONVERGED = 32,"
                     r"\s+HRP_KF_AT_LIMIT = 64", src)
    assert (nv.KF_INIT, nv.KF_COASTED, nv.KF_LOST, nv.KF_BAD_START, nv.KF_REWRAPPED, nv.KF_CONVERGED, nv.KF_AT_LIMIT) == \
        (kf.INIT, kf.COASTED, kf.LOST, kf.BAD_START, kf.REWRAPPED, kf.CONVERGED, kf.AT_LIMIT) == (1, 2, 4, 8, 16, 32, 64)
    assert re.search(r"#define HRP_KIN_FILTER_MAX_N 20\b", src) and nv.KIN_FILTER_MAX_N == 20 == kf.MAX_N
    prog = '#include <stdio.h>\n#include "hrp.h"\nint main(void) { printf("%zu\\n", sizeof(hrp_kin_filter_desc)); return 0; }\n'
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")], check=True)
        size = int(subprocess.run([os.path.join(td, "s")], check=True, stdout=subprocess.PIPE, text=True).stdout)
    assert size == ctypes.sizeof(nv.KinFilterDesc) == 280
    lib = nv.lib()

    def step(**kw):
        d = nv.KinFilterDesc()
        for k in ("chain", "pts2d", "K", "q_in", "rot_in", "trans_in", "q_acc", "p0_var", "mean", "cov", "valid", "coast", "q", "rot", "trans"):
            setattr(d, k, 64)
        d.nkp, d.dof, d.rot_dim, d.pose_stride, d.K_stride, d.free_q, d.free_pose, d.root, d.B, d.max_coast = 7, 8, 3, 1, 9, 0x3f, 1, 0, 1, 5
        d.dt, d.gate_chi2 = 1 / 30, 40.0
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.hrp_kin_filter_step(ctypes.byref(d), None)
    assert lib.hrp_kin_filter_step(None, None) == -1 and b"kin_filter_step" in lib.hrp_last_error()
    for bad in (dict(chain=None), dict(pts2d=None), dict(K=None), dict(q_in=None), dict(rot_in=None), dict(trans_in=None), dict(q=None),
                dict(rot=None), dict(trans=None), dict(rot_dim=4), dict(free_q=1 << 8), dict(B=0), dict(nkp=0), dict(nkp=25), dict(dof=33),
                dict(K_stride=3), dict(pose_stride=2), dict(free_pose=2), dict(root=7), dict(root=-1),
                dict(dt=0.0), dict(dt=-1 / 30), dict(dt=float("inf")), dict(dt=float("nan")), dict(gate_chi2=float("nan")),
                dict(free_q=0, free_pose=0), dict(free_q=0x7fff, dof=15), dict(mean=None), dict(cov=None), dict(valid=None), dict(coast=None),
                dict(q_acc=None), dict(p0_var=None), dict(max_coast=-1), dict(w_q=64), dict(q_meas=64)):
        assert step(**bad) == -1, bad
        assert b"kin_filter_step" in lib.hrp_last_error(), (bad, lib.hrp_last_error())
