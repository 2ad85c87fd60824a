"""CPU-only checks of the kinematic smoother (hrp_kin_smooth): tests/kinsmooth_host_check.cpp runs csrc/kin_smooth_core.h's link_one and
walk_one - the very loops the kernels run - one lane at a time, built with the host compiler and -fsanitize=address,undefined
-fno-sanitize-recover as a plain executable with exact-size buffers.  The golden sequences' replayed histories, the synthetic cases,
hostile inputs, the fixture's own claims, the oracle against a batch solution, the Python surface's refusals (reached before any GPU
call), the C ABI's refusals and the ctypes mirror."""
import ctypes
import inspect
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import hrpe_amd  # noqa: F401
import kinfilter_oracle as kf
import kinsmooth_oracle as ks
from hrpe_amd import _native as nv
from hrpe_amd.lib.utils import kinfit
from hrpe_amd.lib.utils.urdf_robot import URDFRobot

_ROBOTS = {}
FIXTURE = os.path.join(GOLDEN, "golden_kinsmooth.npz")
CLAIMED = ("smooth", "dropout", "outlier", "limit", "holistic")


def robot_of(name):
    if name not in _ROBOTS:
        _ROBOTS[name] = URDFRobot(name)
    return _ROBOTS[name]


@pytest.fixture(scope="module")
def figures():
    return ks.load_fixture(FIXTURE)


@pytest.fixture(scope="module")
def sequences():
    """{name: (seq, history of the oracle's replayed states)}."""
    seqs = kf.load_fixture(os.path.join(GOLDEN, "golden_kinfilter.npz"), lambda n: robot_of(n).chain)
    out = {}
    for name, seq in seqs.items():
        res = kf.replay(seq)
        out[name] = (seq, ks.history_of([s for s, _ in res], [o["flags"] for _, o in res], [seq["filter"].dt] * len(res)))
    return out


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("kinsmooth_host")
    exe = str(td / "kinsmooth_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "kinsmooth_host_check.cpp"), "-o", exe], check=True)
    return exe, td


def run_cases(check_exe, packed, items, tag):
    exe, td = check_exe
    src, dst = str(td / f"{tag}.in"), str(td / f"{tag}.out")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(packed)) + b"".join(packed))
    r = subprocess.run([exe, "run", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return ks.unpack_cases(open(dst, "rb").read(), items)


def test_fixture_is_small_and_states_what_the_issue_claims(figures, sequences):
    assert os.path.getsize(FIXTURE) < 64 * 1024
    assert list(figures) == kf.sequence_names() + list(ks.synthetic_cases())
    for name, (seq, hist) in sequences.items():
        kind, fig = name.split("_", 1)[1], figures[name]
        ref = ks.rts(hist, seq["filter"].q_acc)
        assert np.array_equal(ref["flags"], fig["flags"]) and np.array_equal(ref["count"], fig["count"]), name
        if kind in CLAIMED:
            assert fig["err"][1] < fig["err"][0], name
            assert fig["flags"].tolist() == [ks.SMOOTHED] * 11 + [ks.TAIL], name
        if kind == "limit":
            assert fig["beyond"] > 1e-6, name
        if kind == "restart":
            assert fig["flags"][5] == ks.TAIL and fig["count"][6] == 5, name
        if kind == "lost":
            assert fig["flags"][6] == ks.INVALID and fig["flags"][5] == ks.TAIL, name
        assert 0 < fig["own"][0] < 1e-11 and 0 < fig["own"][1] < 1e-10, (name, fig["own"])
        for t in range(12):
            if not ref["flags"][t] & ks.INVALID:
                assert np.linalg.eigvalsh(ref["cov"][t]).min() > 0, (name, t)
    assert figures["cuts"]["flags"].tolist() == [1, 1, 2, 1, 1, 2, 1, 1, 2, 4, 1, 2, 10, 1, 1, 2]


def test_oracle_against_the_batch_solution_and_80_bit():
    """rts' means are the weighted least-squares solution over the whole sequence; its two float64 formulations agree with the 80-bit
    one to the stored figures' order."""
    for n, L, seed in ((1, 6, 0), (4, 16, 3)):
        hist, q_acc, toy = ks.synthetic(n, L, seed, return_toy=True)
        assert np.abs(ks.rts(hist, q_acc)["mean"] - ks.batch_wls(hist, q_acc, toy)).max() < 1e-9
        fig = ks.own_figures(hist, q_acc)
        assert fig[0] < 1e-11 and fig[1] < 1e-10, fig
    assert np.finfo(np.longdouble).nmant >= 63 or not ks.HAVE_LD


def test_golden_histories_on_the_host(check_exe, sequences, figures):
    worst = np.zeros(4)
    for name, (seq, hist) in sequences.items():
        F, chain = seq["filter"], robot_of(seq["robot"]).chain
        P, L = F.P, len(seq["frames"])
        q_in = np.stack([fr["q_in"] for fr in seq["frames"]])
        fr0 = seq["frames"][0]
        pose = None if P.free_pose else (fr0["rot_in"], fr0["trans_in"])
        ref = ks.rts(hist, F.q_acc)
        packed = [ks.pack_case(chain, P.free, P.free_pose, P.root, 3, ks.in_ring(hist, L, 0), q_in, pose, P.lo, P.hi, F.q_acc, L, 0, L, wc)
                  for wc in (1, 0)]
        got, nocov = run_cases(check_exe, packed, [(F.n, F.dof, F.nkp, 3, L, 1), (F.n, F.dof, F.nkp, 3, L, 0)], name)
        fig = ks.check(name, got, ref, figures[name]["own"], F, q_in, pose)
        for k in ("q", "rot", "trans", "vel", "xyz", "status", "mean"):
            assert got[k].tobytes() == nocov[k].tobytes(), (name, k)
        print(f"{name}: fp64 mean {fig[0]:.1e} cov {fig[1]:.1e} (oracle alone {figures[name]['own'][0]:.1e} {figures[name]['own'][1]:.1e}); "
              f"fp32 parameters {fig[2]:.1e} kp3d {fig[3]:.1e}")
        worst = np.maximum(worst, fig)
    print("largest:", worst)


def test_synthetic_cases_on_the_host(check_exe, figures):
    for name, c in ks.synthetic_cases().items():
        chain = robot_of(c["robot"]).chain
        n, L = len(c["q_acc"]), len(c["hist"]["dt"])
        F = kf.Filter(chain, c["free"], c["free_pose"], 0, np.eye(3), 1 / 30, c["q_acc"], np.ones(2 * n))
        q_in = np.float32(np.random.default_rng(L).uniform(-1, 1, (L, F.dof)))
        ring_q = np.full((c["cap"], F.dof), np.nan, np.float32)
        ring_q[(c["first"] + np.arange(L)) % c["cap"]] = q_in
        pose = None if c["free_pose"] else (np.float32([0.3, -0.2, 0.1]), np.float32([0.05, -0.1, 1.5]))
        ref = ks.rts(c["hist"], c["q_acc"])
        assert np.array_equal(ref["flags"], figures[name]["flags"]) and np.array_equal(ref["count"], figures[name]["count"]), name
        packed = ks.pack_case(chain, c["free"], c["free_pose"], 0, 3, ks.in_ring(c["hist"], c["cap"], c["first"]), ring_q, pose, None, None,
                              c["q_acc"], c["cap"], c["first"], L, 1)
        got, = run_cases(check_exe, [packed], [(n, F.dof, F.nkp, 3, L, 1)], name)
        fig = ks.check(name, got, ref, figures[name]["own"], F, q_in, pose)
        print(f"{name}: fp64 mean {fig[0]:.1e} cov {fig[1]:.1e} (oracle alone {figures[name]['own'][0]:.1e} {figures[name]['own'][1]:.1e})")
        # the newest frames alone: the last rows of everything, byte for byte
        lag = max(1, L // 2)
        part, = run_cases(check_exe, [ks.pack_case(chain, c["free"], c["free_pose"], 0, 3, ks.in_ring(c["hist"], c["cap"], c["first"]), ring_q, pose,
                                                   None, None, c["q_acc"], c["cap"], (c["first"] + L - lag) % c["cap"], lag, 1)],
                          [(n, F.dof, F.nkp, 3, lag, 1)], name + "_lag")
        for k in got:
            assert part[k].tobytes() == got[k][L - lag:].tobytes(), (name, k)


def test_hostile_inputs(check_exe):
    exe, _ = check_exe
    r = subprocess.run([exe, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "failures 0", r.stdout
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("hostile "):
            got[ln.split(":")[0][8:]] = ln.split(":", 1)[1].split()
    field = lambda name, key: got[name][got[name].index(key) + 1]      # noqa: E731
    status = lambda name: [tuple(int(v) for v in s.split("/")) for s in field(name, "status").split(",")]      # noqa: E731
    S, T, I, Bd, Cl = ks.SMOOTHED, ks.TAIL, ks.INVALID, ks.BAD_LINK, ks.CLAMPED
    assert status("plain") == [(S, 5), (S, 4), (S, 3), (S, 2), (S, 1), (T, 0)]
    assert status("NaN mean") == [(S, 2), (S, 1), (T, 0), (I, 0), (S, 1), (T, 0)] == status("NaN row in cov")
    assert status("NaN off the diagonal of cov") == [(S, 3), (S, 2), (S, 1), (T | Bd, 0), (S, 1), (T, 0)]
    assert status("zero row in cov")[3] in ((S, 2), (T | Bd, 0)) and status("zero row in cov")[2][0] == S
    assert status("zero pivot in P-") == [(S, 2), (S, 1), (T | Bd, 0), (S, 2), (S, 1), (T, 0)]
    assert status("dt denormal") == status("plain")
    assert status("dt 1e300") == [(S, 2), (S, 1), (T | Bd, 0), (S, 2), (S, 1), (T, 0)] == status("dt NaN")
    assert status("every frame invalid") == [(I, 0)] * 6
    assert status("beyond a bound") == [(S | Cl, 5), (S | Cl, 4), (S | Cl, 3), (S | Cl, 2), (S | Cl, 1), (T | Cl, 0)]
    assert status("L 1") == [(T, 0)] and status("first = cap - 1") == [(S, 4), (S, 3), (S, 2), (S, 1), (T, 0)]
    assert status("n 1") == [(S, 3), (S, 2), (S, 1), (T, 0)] == status("n 20 nkp 24") == status("n 20 rot_dim 6 root 23 no cov")
    assert status("dof 0") == [(S, 2), (S, 1), (T, 0)] and status("broken chain table") == status("plain")
    for name in ("L 0", "L > cap", "first = cap", "n 21", "n 0", "rot_dim 4", "nkp 25", "free_q beyond dof", "no fixed pose"):
        assert field(name, "refused") == "1", name
    for name, row in got.items():
        if field(name, "refused") == "0":
            assert field(name, "written") == "1", name
            if name != "NaN off the diagonal of cov":      # a usable frame (its diagonal is finite) whose bytes a tail hands on as they are
                assert field(name, "finite32") == "1" and field(name, "symmetric") == "1", name


def test_surface_refuses_before_any_gpu_call():
    import torch
    panda = robot_of("panda")
    cTr = np.array([1.2, -1.0, 0.8, 0.05, -0.1, 1.5])
    f = kinfit.KinematicFilter(panda, "fixed_camera", 1 / 30, 10.0, 0.01, cTr=cTr)
    assert f.history == 0
    with pytest.raises(nv.HrpError, match="nothing is recorded"):
        f.smooth()
    for bad in (-1, 1.5, True):
        with pytest.raises(nv.HrpError, match="history"):
            f.history = bad
    f.history = 12
    assert f.history == 12 and f._hist is None
    with pytest.raises(nv.HrpError, match="empty"):
        f.smooth()
    f.clear_history()
    with pytest.raises(nv.HrpError, match="no CPU path"):
        f.step(torch.zeros(1, 7, 2), torch.eye(3), torch.zeros(1, 8))
    assert f.mean is None and f._hist is None                  # nothing was created on a device
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)      # noqa: E731
    hist = kinfit.KinHistory(z(4, 1, 12), z(4, 1, 12, 12), z(4, 1, dt=torch.int32), z(4, 1, dt=torch.int32), z(4), z(4, 1, 8, dt=torch.float32))
    free = np.arange(8) < 6
    with pytest.raises(nv.HrpError, match="no CPU path"):
        kinfit.kin_smooth(panda, hist, 10.0, free, free_pose=False, pose=(torch.zeros(3), torch.zeros(3)))
    for kw, what in ((dict(free=np.ones(3, bool)), "free"), (dict(free=np.zeros(8, bool)), "parameters"), (dict(q_acc=-1.0), "q_acc"),
                     (dict(root=7), "root"), (dict(rot_dim=4), "rot_dim")):
        args = dict(q_acc=10.0, free=free, free_pose=False)
        args.update(kw)
        with pytest.raises(nv.HrpError, match=what):
            kinfit.kin_smooth(panda, hist, args.pop("q_acc"), args.pop("free"), **args)
    p = inspect.signature(kinfit.KinematicFilter.smooth).parameters
    assert list(p) == ["self", "lag", "cov", "full"] and [p[k].default for k in list(p)[1:]] == [None, True, False]
    assert kinfit.KinSmoothResult._fields == ("q", "rot", "trans", "vel", "cov", "kp3d", "status", "mean", "cov_full")
    assert kinfit.KinHistory._fields == ("mean", "cov", "valid", "flags", "dt", "q_in")


def test_smoother_abi_declared_bound_and_refusing():
    src = open(os.path.join(ROOT, "include", "hrp.h")).read()
    assert re.search(r"\bint\s+hrp_kin_smooth\s*\(\s*const hrp_kin_smooth_desc\*", src) and len(nv.PROTOTYPES["hrp_kin_smooth"]) == 2
    assert re.search(r"\bint\s+hrp_kin_history_push\s*\(\s*const hrp_kin_history_desc\*", src) and len(nv.PROTOTYPES["hrp_kin_history_push"]) == 2
    assert re.search(r"HRP_KS_SMOOTHED = 1, HRP_KS_TAIL = 2, HRP_KS_INVALID = 4, HRP_KS_BAD_LINK = 8, HRP_KS_CLAMPED = 16", src)
    assert (nv.KS_SMOOTHED, nv.KS_TAIL, nv.KS_INVALID, nv.KS_BAD_LINK, nv.KS_CLAMPED) == \
        (ks.SMOOTHED, ks.TAIL, ks.INVALID, ks.BAD_LINK, ks.CLAMPED) == (1, 2, 4, 8, 16)
    prog = ('#include <stdio.h>\n#include "hrp.h"\nint main(void) { printf("%zu %zu\\n", sizeof(hrp_kin_smooth_desc), '
            'sizeof(hrp_kin_history_desc)); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")], check=True)
        sizes = [int(v) for v in subprocess.run([os.path.join(td, "s")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(nv.KinSmoothDesc), ctypes.sizeof(nv.KinHistoryDesc)] == [232, 120]
    lib = nv.lib()

    def smooth(**kw):
        d = nv.KinSmoothDesc()
        for k in ("chain", "mean", "cov", "valid", "flags", "dt", "q_in", "rot_fixed", "trans_fixed", "q_acc", "gain", "link", "q", "rot", "trans",
                  "vel", "cov_p", "xyz", "status"):
            setattr(d, k, 64)
        d.free_q, d.free_pose, d.root, d.B, d.dof, d.nkp, d.rot_dim, d.cap, d.first, d.L, d.want_cov = 0x3f, 0, 0, 1, 8, 7, 3, 8, 0, 8, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.hrp_kin_smooth(ctypes.byref(d), None)
    assert lib.hrp_kin_smooth(None, None) == -1 and b"kin_smooth" in lib.hrp_last_error()
    for bad in (dict(chain=None), dict(mean=None), dict(cov=None), dict(valid=None), dict(flags=None), dict(dt=None), dict(q_in=None),
                dict(q_acc=None), dict(gain=None), dict(link=None), dict(q=None), dict(rot=None), dict(trans=None), dict(vel=None),
                dict(xyz=None), dict(status=None), dict(cov_p=None), dict(rot_fixed=None), dict(trans_fixed=None), dict(B=0), dict(L=0),
                dict(L=9), dict(cap=0), dict(first=8), dict(first=-1), dict(free_q=0), dict(free_q=0x7fff, dof=15, free_pose=1),
                dict(dof=33), dict(dof=-1), dict(nkp=0), dict(nkp=25), dict(free_q=1 << 8), dict(root=7), dict(root=-1), dict(rot_dim=4),
                dict(free_pose=2)):
        assert smooth(**bad) == -1, bad
        assert b"kin_smooth" in lib.hrp_last_error(), (bad, lib.hrp_last_error())

    def push(**kw):
        d = nv.KinHistoryDesc()
        for k in ("mean", "cov", "valid", "status", "q_in", "h_mean", "h_cov", "h_valid", "h_flags", "h_dt", "h_q_in"):
            setattr(d, k, 64)
        d.B, d.n, d.dof, d.cap, d.slot, d.dt = 1, 6, 8, 4, 0, 1 / 30
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.hrp_kin_history_push(ctypes.byref(d), None)
    assert lib.hrp_kin_history_push(None, None) == -1 and b"kin_history_push" in lib.hrp_last_error()
    for bad in (dict(mean=None), dict(cov=None), dict(valid=None), dict(status=None), dict(q_in=None), dict(h_mean=None), dict(h_cov=None),
                dict(h_valid=None), dict(h_flags=None), dict(h_dt=None), dict(h_q_in=None), dict(B=0), dict(n=0), dict(n=21), dict(dof=33),
                dict(cap=0), dict(slot=4), dict(slot=-1), dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("inf"))):
        assert push(**bad) == -1, bad
        assert b"kin_history_push" in lib.hrp_last_error(), (bad, lib.hrp_last_error())
