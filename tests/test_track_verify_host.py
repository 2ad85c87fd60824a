"""CPU-only checks of the tracker's verification step (track_verify, csrc/track_core.h) under tests/track_verify_host_check.cpp,
built with the host compiler and -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off (a plain executable): the
rule of include/hrp.h against the float64 numpy statement of tests/track_verify_oracle.py on maps of exactly hm * wm floats
(status, have and the four counts equal, the state's bits unchanged, I / S / R equal on binary maps and within hm * wm * 2^-53
otherwise), the host refusals of hrp_track_verify, PoseTracker's argument checks, and the constants and the descriptor's layout
against a C program."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
import track_verify_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("track_verify_host")
    exe = str(td / "track_verify_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "track_verify_host_check.cpp"), "-o", exe], check=True)
    return exe, td


def pack(c):
    nkp, (hm, wm) = len(c["state"]), c["mask"].shape
    head = np.array([nkp, c["have"], hm, wm, c["alpha"] is not None, len(c["bones"]), c["samples"], c["min_fg"], c["min_samples"]], np.int32)
    blob = head.tobytes() + np.float32(c["min_prob"]).tobytes()
    blob += np.array(list(c["scale"]) + list(c["extend_ratio"]) + [c["min_support"], c["min_coverage"], c["min_iou"]], np.float64).tobytes()
    blob += np.asarray(c["bones"], np.int32).reshape(-1, 2).tobytes() + c["mask"].tobytes()
    if c["alpha"] is not None:
        blob += c["alpha"].tobytes()
    return blob + np.ascontiguousarray(c["state"], np.float64).tobytes()


def test_verify_equals_numpy_under_the_sanitizers(check_exe):
    exe, td = check_exe
    cases = O.cases()
    src, dst = td / "verify.in", td / "verify.out"
    src.write_bytes(np.int32(len(cases)).tobytes() + b"".join(pack(c) for c in cases))
    r = subprocess.run([exe, "run", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    raw, off, seen = dst.read_bytes(), 0, set()
    for n, c in enumerate(cases):
        nkp, (hm, wm) = len(c["state"]), c["mask"].shape
        st, have, *counts = np.frombuffer(raw, np.int32, 6, off).tolist()
        sums = np.frombuffer(raw, np.float64, 3, off + 24)
        state = np.frombuffer(raw, np.float64, 2 * nkp, off + 48).reshape(nkp, 2)
        off += 48 + 16 * nkp
        w_st, w_have, w_counts, w_sums = O.verify(**O.call_args(c))
        assert (st, have, counts) == (w_st, w_have, w_counts.tolist()), (n, st, have, counts, w_st, w_have, w_counts)
        assert np.array_equal(state.view(np.uint64), c["state"].view(np.uint64)), n                       # never written
        assert O.sums_ok(sums, w_sums, hm * wm, c["exact"]), (n, sums, w_sums)
        seen.add(w_st)
    assert off == len(raw) and seen == O.ALL_OUTCOMES, sorted(seen)
    # every axis of the generator was visited
    assert {len(c["state"]) for c in cases} >= {1, 7, 32} and {c["samples"] for c in cases} >= {1, 16, 64}
    assert {len(c["bones"]) for c in cases} >= {0, 6, 31, O.MAX_BONES} and {c["mask"].shape for c in cases} >= set(O.SIZES)
    assert {(c["alpha"] is not None, c["exact"]) for c in cases} == {(a, e) for a in (False, True) for e in (False, True)}


def _desc(**over):
    """A descriptor that passes every host check (the pointers are never followed on the host)."""
    d = nv.TrackVerifyDesc()
    d.state_kp2d, d.state_have, d.mask, d.alpha, d.verify_status, d.counts, d.sums = 64, 64, 64, 64, 64, 64, 64
    d.B, d.nkp, d.hm, d.wm, d.nb, d.samples, d.min_fg, d.min_samples = 2, 7, 240, 320, 6, 16, 16, 4
    for i in range(6):
        d.bones[i][0], d.bones[i][1] = i, i + 1
    d.scale[0], d.scale[1], d.extend_ratio[0], d.extend_ratio[1] = 0.5, 0.5, 0.2, 0.13
    d.min_support, d.min_coverage, d.min_iou, d.min_prob = 0.5, 0.5, 0.5, 0.5
    for k, v in over.items():
        if k == "bone":
            d.bones[v[0]][0], d.bones[v[0]][1] = v[1], v[2]
        elif k in ("scale", "extend_ratio"):
            getattr(d, k)[0], getattr(d, k)[1] = v
        else:
            setattr(d, k, v)
    return d


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = nv.lib()
    nan, inf = float("nan"), float("inf")
    bad = [dict(state_kp2d=None), dict(state_have=None), dict(mask=None), dict(verify_status=None), dict(counts=None), dict(sums=None),
           dict(B=0), dict(B=65536), dict(nkp=0), dict(nkp=33), dict(hm=0), dict(wm=0), dict(hm=4097), dict(wm=4097), dict(nb=-1),
           dict(nb=nv.TRACK_MAX_BONES + 1), dict(bone=(2, 0, 7)), dict(bone=(5, -1, 3)), dict(samples=0), dict(samples=65),
           dict(scale=(nan, 0.5)), dict(scale=(0.5, inf)), dict(scale=(0.0, 0.5)), dict(scale=(0.5, -0.5)), dict(extend_ratio=(nan, 0.1)),
           dict(extend_ratio=(0.2, -inf)), dict(min_support=1.5), dict(min_coverage=nan), dict(min_iou=1.0000001), dict(min_support=nan),
           dict(alpha=None), dict(alpha=None, min_iou=0.0), dict(mask=66), dict(sums=68)]
    for over in bad:
        assert lib.hrp_track_verify(C.byref(_desc(**over)), None) == -1, over
        assert b"track_verify" in lib.hrp_last_error(), over
    assert lib.hrp_track_verify(None, None) == -1 and b"track_verify" in lib.hrp_last_error()
    with pytest.raises(nv.HrpError, match="track_verify"):
        nv.call("hrp_track_verify", C.byref(_desc(nkp=33)), None)


def test_constants_and_descriptor_layout(check_exe):
    exe, _ = check_exe
    got = [int(v) for v in subprocess.run([exe, "sizeof"], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    D = nv.TrackVerifyDesc
    assert got[:5] == [C.sizeof(D), D.B.offset, D.bones.offset, D.scale.offset, D.min_prob.offset] == [408, 56, 88, 344, 400]
    assert got[5:] == [nv.VERIFY_SKIPPED, nv.VERIFY_KEPT, nv.VERIFY_UNDECIDED, nv.VERIFY_DROPPED, nv.VERIFY_FAIL_SUPPORT, nv.VERIFY_FAIL_COVERAGE,
                       nv.VERIFY_FAIL_IOU, nv.TRACK_MAX_BONES, nv.TRACK_MAX_SAMPLES]
    assert got[5:] == [O.SKIPPED, O.KEPT, O.UNDECIDED, O.DROPPED, O.FAIL_SUPPORT, O.FAIL_COVERAGE, O.FAIL_IOU, O.MAX_BONES, O.MAX_SAMPLES]
    assert "hrp_track_verify" in nv.PROTOTYPES and hasattr(nv.lib(), "hrp_track_verify")


def test_tracker_arguments_without_a_gpu():
    """The verification arguments are checked on the host, before the device is looked at."""
    from hrpe_amd.lib.core.tracker import PoseTracker
    K = np.array([[615.0, 0, 320], [0, 615, 240], [0, 0, 1]])
    det, rnd = (lambda x: x), object()
    robot = types.SimpleNamespace(nkp=7, robot_type="panda")
    for kw, what in ((dict(detector=det, min_support=1.5), "min_support"), (dict(detector=det, min_coverage=-0.1), "min_coverage"),
                     (dict(detector=det, min_iou=float("nan"), renderer=rnd), "min_iou"), (dict(min_support=0.5), "detector"),
                     (dict(detector=det, min_iou=0.5), "renderer"), (dict(detector=det, min_support=0.5, renderer=rnd), "renderer"),
                     (dict(detector=det, min_support=0.5, bones=[(0, 7)]), "bones"), (dict(detector=det, min_support=0.5, bones=[(-1, 2)]), "bones"),
                     (dict(detector=det, min_support=0.5, bones=[(0, 1, 2)]), "bones"), (dict(detector=det, min_support=0.5, bones=[(0, 1)] * 33), "bones"),
                     (dict(detector=det, min_support=0.5, verify_samples=65), "verify_samples")):
        with pytest.raises(nv.HrpError, match=what):
            PoseTracker(lambda *a: None, robot, K, (480, 640), device="cpu", **kw)
    with pytest.raises(nv.HrpError, match="K_original"):
        PoseTracker(lambda *a: None, robot, np.stack([K, K]), (480, 640), streams=2, device="cpu", detector=det, min_iou=0.5, renderer=rnd)
    for kw in (dict(min_support=0.5), dict(min_coverage=0.0, bones=[(0, 6)]), dict(min_iou=1.0, renderer=rnd)):    # good: only the device is missing
        with pytest.raises(nv.HrpError, match="not a GPU"):
            PoseTracker(lambda *a: None, robot, K, (480, 640), device="cpu", detector=det, **kw)
