"""CPU-only checks of the pooled robust PnP (hrp_pnp_solve_pooled): tests/pnp_pooled_host_check.cpp restates the loop of
csrc/pnp_pooled.hip over csrc/pnp_minimal.h and is built with the host compiler and -fsanitize=address,undefined
-fno-sanitize-recover as a plain executable.  The capped 64-bit hypothesis count, the sampled triples at m = 16384, hostile inputs, the
whole loop on every case of golden_pnp_pooled.npz, the fixture's own conditions, the C ABI's refusals and the Python surface."""
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
from hrpe_amd import _native as nv

POOLED_CASES = {"f10x7": (10, 7), "f37x7": (37, 7), "f150x7": (150, 7), "f9x17": (9, 17)}


def load_pooled():
    return np.load(os.path.join(GOLDEN, "golden_pnp_pooled.npz"))


def pooled_case(g, c):
    """(pts2d [n,2], pts3d [n,3], K, P6d, P6d_all, mask [n] bool) of case c, the frames laid end to end, float64."""
    x, X, K, P, Pa = (g[f"{c}_{k}"].astype(np.float64) for k in ("pts2d", "pts3d", "K", "P6d", "P6d_all"))
    return x.reshape(-1, 2), X.reshape(-1, 3), K, P, Pa, g[f"{c}_mask"].astype(bool).ravel()


def reprojection_errors(P, X, x, K):
    from test_pnp_host import rodrigues_np
    cam = X @ rodrigues_np(P[None, :3])[0].T + P[3:]
    p = cam @ K.T
    return np.sqrt(((p[:, :2] / p[:, 2:3] - x) ** 2).sum(-1)), cam[:, 2]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("pnp_pooled_host")
    exe = str(td / "pnp_pooled_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "pnp_pooled_host_check.cpp"), "-o", exe], check=True)
    return exe, td


@pytest.fixture(scope="module")
def self_output(check_exe):
    exe, _ = check_exe
    r = subprocess.run([exe, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().splitlines()[-1] == "failures 0", r.stdout
    return r.stdout


def test_capped_count_beyond_int(self_output):
    """ncomb3_capped equals ncomb3 for m <= 64 (checked inside) and is C(m, 3) at 2343, 2344 and 16384, where ncomb3's int product
    has long wrapped."""
    got = {int(ln.split()[2][:-1]): int(ln.split()[3]) for ln in self_output.splitlines() if ln.startswith("count m")}
    assert got == {m: m * (m - 1) * (m - 2) // 6 for m in (2343, 2344, 16384)}


def test_sampled_triples_at_the_largest_size(self_output):
    w = [ln for ln in self_output.splitlines() if ln.startswith("sampled m 16384")][0].split()
    assert int(w[3]) == 0, w


def test_hostile_inputs_report_m(self_output):
    lines = [ln for ln in self_output.splitlines() if ln.startswith("hostile")]
    assert lines == ["hostile non-finite: m 64 H 1024 count 64", "hostile three points: m 3 H 0 count -1 rounds 0"], lines


def test_fixture_conditions():
    """What gen_golden_pnp_pooled.py asserts, checked again on the committed file."""
    g = load_pooled()
    assert os.path.getsize(os.path.join(GOLDEN, "golden_pnp_pooled.npz")) < 128 * 1024
    assert list(g["cases"]) == list(POOLED_CASES)
    total = 0
    for c, (F, k) in POOLED_CASES.items():
        assert g[f"{c}_pts2d"].shape == (F, k, 2) and g[f"{c}_pts3d"].shape == (F, k, 3) and g[f"{c}_mask"].shape == (F, k)
        x, X, K, P, Pa, mask = pooled_case(g, c)
        total += len(x)
        e, depth = reprojection_errors(P, X, x, K)
        assert e[mask].max() < 2 and e[~mask].min() > 10, (c, e[mask].max(), e[~mask].min())
        assert depth.min() > 0 and reprojection_errors(Pa, X, x, K)[1].min() > 0
        gap = max(np.abs(P[3:] - Pa[3:]).max(), np.sqrt(((P[:3] - Pa[:3]) ** 2).sum()))
        assert gap > 1e-3, (c, gap)
        whole = ~g[f"{c}_mask"].astype(bool).any(1)
        assert whole.sum() == round(0.3 * F), (c, whole.sum())        # the frames displaced as a whole
    assert total == 1532


def test_whole_loop_ends_on_the_planted_mask(check_exe):
    """Every case: compaction, hypotheses, scoring, the winner, then the re-score loop with the fixture's optimum in place of the LM
    refit.  The winner's consensus holds no planted outlier and at least min_inliers points, and the loop ends on exactly the
    planted mask within HRP_PNP_POOLED_REFITS rounds."""
    exe, td = check_exe
    g = load_pooled()
    blob, want = [], []
    min_inliers = 4
    for c in POOLED_CASES:
        x, X, K, P, _, mask = pooled_case(g, c)
        n = len(x)
        blob.append(np.array([n, 1024, 0, min_inliers], np.int32).tobytes() + np.float64(3.0).tobytes() +
                    b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (K, X, x, P)) + np.ones(n, np.uint8).tobytes())
        want.append((c, mask))
    src, dst = td / "loop.in", td / "loop.out"
    src.write_bytes(np.int32(len(blob)).tobytes() + b"".join(blob))
    r = subprocess.run([exe, "loop", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    raw, off = dst.read_bytes(), 0
    for c, mask in want:
        n = len(mask)
        m, H, count, rounds = np.frombuffer(raw[off:off + 16], np.int32)
        m0 = np.frombuffer(raw[off + 16:off + 16 + n], np.uint8)
        m1 = np.frombuffer(raw[off + 16 + n:off + 16 + 2 * n], np.uint8)
        off += 16 + 2 * n
        print(f"{c}: m {m}, H {H}, the winner holds {count} of {mask.sum()} planted inliers, {rounds} rounds")
        assert m == n and H == 1024, (c, m, H)
        assert count == m0.sum() >= min_inliers and not (m0 & ~mask).any(), (c, count)
        assert np.array_equal(m1.astype(bool), mask), (c, np.flatnonzero(m1.astype(bool) != mask))
        assert 1 <= rounds <= nv.PNP_POOLED_REFITS, (c, rounds)
    assert off == len(raw)


def test_pooled_abi_declared_bound_and_refusing():
    src = open(os.path.join(ROOT, "include", "hrp.h")).read()
    for name in ("hrp_pnp_solve_pooled", "hrp_pnp_pooled_workspace_bytes"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in nv.PROTOTYPES
    assert len(nv.PROTOTYPES["hrp_pnp_solve_pooled"]) == 20 and len(nv.PROTOTYPES["hrp_pnp_pooled_workspace_bytes"]) == 4
    assert re.search(r"HRP_PNP_POOLED_MAX_N\s*=\s*16384\b", src) and nv.PNP_POOLED_MAX_N == 16384
    assert re.search(r"HRP_PNP_POOLED_REFITS\s*=\s*8\b", src) and nv.PNP_POOLED_REFITS == 8
    assert len(nv.PROTOTYPES["hrp_pnp_solve_robust"]) == 18            # the existing entry point keeps its arguments
    lib = nv.lib()
    need = ctypes.c_size_t(0)
    assert lib.hrp_pnp_pooled_workspace_bytes(1, 70, 1024, ctypes.byref(need)) == 0 and need.value >= 16 + 4 * 70 + 1024 * 112
    big = ctypes.c_size_t(0)
    assert lib.hrp_pnp_pooled_workspace_bytes(3, 16384, 1024, ctypes.byref(big)) == 0 and big.value % 3 == 0 and big.value > 3 * 4 * 16384
    assert lib.hrp_pnp_pooled_workspace_bytes(1, 16385, 1024, ctypes.byref(big)) == -1
    assert b"pnp_pooled_workspace_bytes" in lib.hrp_last_error()

    def solve(n=70, thr=3.0, min_inliers=4, max_hypotheses=1024, ws=64, ws_bytes=None):
        return lib.hrp_pnp_solve_pooled(64, 64, 64, 0, None, 1, n, thr, min_inliers, max_hypotheses, 0, 0, ws,
                                        need.value if ws_bytes is None else ws_bytes, 64, 64, 64, 64, None, None)
    for bad in (dict(n=3), dict(n=16385), dict(thr=0.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(min_inliers=3),
                dict(min_inliers=71), dict(max_hypotheses=0), dict(max_hypotheses=(1 << 20) + 1), dict(ws_bytes=need.value - 1),
                dict(ws=None)):
        assert solve(**bad) == -1, bad
        assert b"pnp_solve_pooled" in lib.hrp_last_error(), (bad, lib.hrp_last_error())
    # the robust solver still refuses what it refused
    assert lib.hrp_pnp_solve_robust(64, 64, 0, 64, 0, None, 1, 65, 3.0, 4, 1024, 0, 0, 64, 64, 64, 64, None) == -1


def test_module_surface():
    from hrpe_amd.lib.core.calibrate import CalibrationResult, CameraCalibrator
    from hrpe_amd.lib.models.ctrnet.CtRNet import CtRNet
    from hrpe_amd.lib.utils import BPnP as M
    p = inspect.signature(M.pnp_solve_pooled).parameters
    assert list(p) == ["pts2d", "pts3d", "K", "reproj_error", "valid", "min_inliers", "max_hypotheses", "seed", "refine_all", "want_cov"]
    assert [p[k].default for k in list(p)[3:]] == [3.0, None, 4, 1024, 0, False, True]
    p = inspect.signature(CameraCalibrator.__init__).parameters
    assert list(p) == ["self", "robot", "K", "capacity_frames", "reproj_error", "min_inliers", "max_hypotheses", "seed", "device"]
    assert [p[k].default for k in list(p)[3:]] == [1024, 3.0, None, 1024, 0, "cuda"]
    assert list(inspect.signature(CameraCalibrator.add).parameters) == ["self", "points_2d", "joint_angles", "valid", "points_3d"]
    p = inspect.signature(CameraCalibrator.add_detection).parameters
    assert list(p) == ["self", "kp", "ms", "joint_angles", "scale", "min_peak"] and p["min_peak"].default == 0.0
    assert list(inspect.signature(CameraCalibrator.solve).parameters) == ["self", "refine_all"]
    assert callable(CameraCalibrator.reset) and callable(CameraCalibrator.__len__)
    assert CalibrationResult._fields == ("cTr", "R", "t", "inliers", "frame_inliers", "rms", "cov", "status")
    p = inspect.signature(CtRNet.inference_sequence).parameters
    assert list(p) == ["self", "img", "joint_angles", "points_3d", "reproj_error"] and p["reproj_error"].default == 3.0
