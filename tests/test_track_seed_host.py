"""CPU-only checks of the tracker's acquisition step (track_seed, csrc/track_core.h) under tests/track_seed_host_check.cpp, built
with the host compiler and -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off (a plain executable): the rule of
include/hrp.h against float64 numpy with a bit-equal state, hostile detections (NaN, +-inf, +-1e300, key-points on every side of
the frame, a mask of exactly hm * wm floats, min_inside above nkp, skipped and forced streams), and the argument checks of
hrp_track_seed."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
import track_seed_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("track_seed_host")
    exe = str(td / "track_seed_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "track_seed_host_check.cpp"), "-o", exe], check=True)
    return exe, td


def pack(c):
    nkp = len(c["det"])
    mask, ms = c["mask"], c["ms"]
    hm, wm = mask.shape if mask is not None else (0, 0)
    head = np.array([nkp, c["have"], hm, wm, mask is not None, ms is not None, c["min_inside"], c["force"], c["W"], c["H"]], np.int32)
    blob = head.tobytes() + np.array([c["min_prob"], c["min_peak"]], np.float32).tobytes() + np.array(c["inv"], np.float64).tobytes()
    blob += np.ascontiguousarray(c["det"], np.float32).tobytes()
    blob += np.ascontiguousarray(ms if ms is not None else np.zeros((nkp, 2)), np.float32).tobytes()
    if mask is not None:
        blob += np.ascontiguousarray(mask, np.float32).tobytes()
    return blob + np.ascontiguousarray(c["state"], np.float64).tobytes()


def test_seed_equals_numpy_under_the_sanitizers(check_exe):
    exe, td = check_exe
    cases = O.cases(np.random.default_rng(11)) + O.cases(np.random.default_rng(12), nkp=1, W=33, H=17, hm=17, wm=33)[:5] \
        + O.cases(np.random.default_rng(13), nkp=32, W=4096, H=4096, hm=64, wm=64)[:8]
    src, dst = td / "seed.in", td / "seed.out"
    src.write_bytes(np.int32(len(cases)).tobytes() + b"".join(pack(c) for c in cases))
    r = subprocess.run([exe, "run", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    raw, off, seen = dst.read_bytes(), 0, set()
    for n, c in enumerate(cases):
        nkp = len(c["det"])
        st, have = np.frombuffer(raw, np.int32, 2, off)
        state = np.frombuffer(raw, np.float64, 2 * nkp, off + 8).reshape(nkp, 2)
        off += 8 + 16 * nkp
        w_st, w_have, w_state = O.seed(**c)
        assert (int(st), int(have)) == (w_st, w_have), (n, st, have, w_st, w_have)
        assert np.array_equal(state.view(np.uint64), np.ascontiguousarray(w_state, np.float64).view(np.uint64)), n   # bit-equal
        seen.add(w_st)
    assert off == len(raw) and seen == {O.SKIPPED, O.TAKEN, O.REFUSED}


def _seed_args(**over):
    """Arguments of hrp_track_seed that pass every host check (the pointers are never followed on the host)."""
    a = dict(det=64, B=1, nkp=7, inv=(C.c_double * 2)(2.0, 2.0), mask=None, hm=0, wm=0, min_prob=0.5, ms=None, min_peak=0.0, min_inside=1,
             force=0, W=640, H=480, kp2d=64, have=64, status=64, stream=None)
    a.update(over)
    return list(a.values())


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = nv.lib()
    nan2, neg2 = (C.c_double * 2)(float("nan"), 2.0), (C.c_double * 2)(2.0, -1.0)
    bad = [dict(det=None), dict(inv=None), dict(kp2d=None), dict(have=None), dict(status=None), dict(B=0), dict(B=65536), dict(nkp=0),
           dict(nkp=33), dict(W=0), dict(H=0), dict(W=4097), dict(H=4097), dict(mask=64, hm=0, wm=320), dict(mask=64, hm=240, wm=4097),
           dict(inv=nan2), dict(inv=neg2)]
    for over in bad:
        assert lib.hrp_track_seed(*_seed_args(**over)) == -1, over
        assert b"track_seed" in lib.hrp_last_error(), over
    with pytest.raises(nv.HrpError):
        nv.call("hrp_track_seed", *_seed_args(nkp=33))
    assert (nv.SEED_SKIPPED, nv.SEED_TAKEN, nv.SEED_REFUSED) == (O.SKIPPED, O.TAKEN, O.REFUSED) == (1, 2, 4)


def test_tracker_arguments_without_a_gpu():
    from hrpe_amd.lib.core.tracker import PoseTracker
    """The detector arguments are checked on the host, before the device is looked at."""
    K = np.array([[615.0, 0, 320], [0, 615, 240], [0, 0, 1]])
    det = lambda x: x   # noqa: E731
    for kw, what in ((dict(acquire_every=2), "acquire_every"), (dict(detector=det, acquire_every=-1), "acquire_every"),
                     (dict(detector=det, detector_scale=0.0), "detector_scale"), (dict(detector=det, detector_scale=(0.5, float("nan"))), "detector_scale"),
                     (dict(detector=det, detector_scale=(0.5, 0.5, 0.5)), "detector_scale")):
        with pytest.raises(nv.HrpError, match=what):
            PoseTracker(lambda *a: None, None, K, (480, 640), device="cpu", **kw)
    with pytest.raises(nv.HrpError, match="not a GPU"):
        PoseTracker(lambda *a: None, None, K, (480, 640), device="cpu", detector=det, detector_scale=(0.5, 0.25), acquire_every=2)
