"""CPU-only checks of the streaming tracker's core (csrc/track_core.h) under tests/track_host_check.cpp, built with the host
compiler and -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off (a plain executable): the geometry against the
DREAM loader on the scene frames, the pixels against the reference's recorded bytes, hostile estimates and wrong records inside
frames allocated at exactly H * W * 3 bytes, and the host-side argument checks of hrp_track_prepare / hrp_track_update."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.dataset import dream as D  # noqa: E402
import dream_scene  # noqa: E402
import track_oracle as O  # noqa: E402
from test_dream_host import CASES, GOLD, need_frame, run_case, scene  # noqa: E402,F401

VIEW_PAIRS = [((128, 128), (128, 128)), ((256, 256), (256, 256)), ((216, 216), (128, 128))]
EXTEND = (0.2, 0.13)
RESULT_BYTES = C.sizeof(nv.TrackGeom) + 4 * 19


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("track_host")
    exe = str(td / "track_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "track_host_check.cpp"), "-o", exe], check=True)
    return exe, td


def pack_case(kp2d, have, K, W, H, root_hw, other_hw, mode, frame=None):
    two = int((min(root_hw), max(root_hw)) != (min(other_hw), max(other_hw)))
    kp2d = np.ascontiguousarray(kp2d, dtype=np.float64)
    head = np.array([W, H, len(kp2d), have, min(root_hw), max(root_hw), min(other_hw), max(other_hw), two, O.MODES[mode]], np.int32)
    blob = head.tobytes() + np.array(EXTEND, np.float64).tobytes() + np.asarray(K, np.float32).tobytes() + kp2d.tobytes()
    return blob + (b"" if frame is None else np.ascontiguousarray(frame, dtype=np.uint8).tobytes()), two


def run_check(check_exe, cmd, cases, name):
    exe, td = check_exe
    src, dst = td / (name + ".in"), td / (name + ".out")
    src.write_bytes(np.int32(len(cases)).tobytes() + b"".join(cases))
    r = subprocess.run([exe, cmd, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return dst.read_bytes()


def split_result(raw):
    g = O.geom_array(raw[:C.sizeof(nv.TrackGeom)])[0]
    f = np.frombuffer(raw[C.sizeof(nv.TrackGeom):RESULT_BYTES], np.float32)
    return g, f[0:9], f[9:18], float(f[18])


def plain_dataset(base, root_hw, other_hw):
    return D.DreamDataset(base, color_jitter=False, rgb_augmentation=False, occlusion_augmentation=False,
                          rootnet_resize_hw=root_hw, other_resize_hw=other_hw)


def item_record(item):
    """A DreamDataset item in the shape of track_oracle.loader_record."""
    a = {k: item["aug"][i].item() for i, k in enumerate(D.AUG_FIELDS)}
    assert all(a[k] == int(a[k]) for k in D.AUG_FIELDS[7:])
    rec = dict(crop=tuple(int(a[k]) for k in ("crop_x0", "crop_y0", "crop_x1", "crop_y1")), side=int(a["side"]),
               off=(int(a["off_x"]), int(a["off_y"])), root=item["root"], other=item["other"],
               strict_original=item["bbox_strict_bounded_original"])
    rec["k"] = {m: O.k_value(m, item["root"], rec["strict_original"], item["K_original"]) for m in O.MODES}
    return rec


def test_geometry_equals_the_loader(scene, check_exe):  # noqa: F811
    """The five scene frames seeded with their annotated projections, three view pairs, three bbox modes: crop box, side and offsets
    equal DreamDataset's ``aug`` record exactly; K, both boxes of both views and k_values within the project's tolerance - of the
    loader's item (true 3-D key-points) and of the ray-based host path the GPU tests use as their oracle."""
    cases, want = [], []
    for root_hw, other_hw in VIEW_PAIRS:
        ds = plain_dataset(scene, root_hw, other_hw)
        for i, spec in enumerate(dream_scene.FRAMES):
            item = ds[i]
            W, H = spec["size"]
            kp2d = np.asarray(item["keypoints_2d_original"], np.float64)
            rec = O.loader_record(kp2d, item["K_original"], W, H, root_hw, other_hw, EXTEND)
            for mode in O.MODES:
                cases.append(pack_case(kp2d, 1, item["K_original"], W, H, root_hw, other_hw, mode)[0])
                want.append((item_record(item), rec, mode, (root_hw, other_hw, i, mode)))
    raw = run_check(check_exe, "geom", cases, "geom")
    assert len(raw) == RESULT_BYTES * len(cases)
    sides = set()
    for n, (irec, rec, mode, where) in enumerate(want):
        g, K_root, K_other, k = split_result(raw[n * RESULT_BYTES:(n + 1) * RESULT_BYTES])
        assert int(g["status"]) == 0, where
        O.check_record(g, K_root, K_other, k, irec, mode, where)
        O.check_record(g, K_root, K_other, k, rec, mode, where)
        sides.add((int(g["side"]), where[0]))
    assert (216, (216, 216)) in sides, "the fixture's side_equals_out case (frame 3, 216 x 216) did not take the copy path"
    crops = {w[3][2]: w[0]["crop"] for w in want}
    assert crops[1][0] == 0 and crops[2][2] == 640 and crops[2][3] == 480, crops            # clamped at the border
    assert crops[3][2] - crops[3][0] == 216 and crops[4][2] <= 400 and crops[4][3] <= 300, crops   # grown by 75 a side; the small frame


def test_loader_stays_within_tolerance_of_the_reference(scene):  # noqa: F811
    """The oracle's own error: the loader's geometry of frame 0 against the reference's recorded ``off`` case, at the tolerance the
    tracker is held to."""
    case = CASES["off"]
    need_frame(scene, case)
    _, item, _ = run_case(scene, case)
    for v in ("root", "other"):
        for k in ("K", "bbox_strict_bounded", "bbox_gt2d_extended"):
            assert np.allclose(item[v][k].numpy(), GOLD["off/" + v + "/" + k], atol=O.ATOL, rtol=O.RTOL), (v, k)
    assert np.allclose(item["bbox_strict_bounded_original"].numpy(), GOLD["off/bbox_strict_bounded_original"], atol=O.ATOL, rtol=O.RTOL)
    assert np.array_equal(item["K_original"], GOLD["off/K_original"])


def test_pixels_equal_the_reference(scene, check_exe):  # noqa: F811
    """track_pixel over the decoded frame 0 with the ``off`` case's key-points: the reference's recorded bytes of both views."""
    case = CASES["off"]
    need_frame(scene, case)
    _, item, _ = run_case(scene, case)
    frame = item["frame"].numpy()
    H, W = frame.shape[:2]
    for other_hw in ((128, 128), (96, 96)):          # one size (written once), and two views: the second walks its own pixels
        blob, two = pack_case(item["keypoints_2d_original"], 1, item["K_original"], W, H, (128, 128), other_hw, "extended", frame)
        raw = run_check(check_exe, "pixels", [blob], "pixels%d" % other_hw[0])
        n0 = 3 * 128 * 128
        root = np.frombuffer(raw[RESULT_BYTES:RESULT_BYTES + n0], np.uint8).reshape(3, 128, 128)
        assert np.array_equal(root, GOLD["off/root/images"])
        want_other = GOLD["off/other/images"] if "off/other/images" in GOLD.files else GOLD["off/root/images"]
        if two:
            other = np.frombuffer(raw[RESULT_BYTES + n0:], np.uint8).reshape(3, *other_hw)
            from test_dream_host import emulate
            assert np.array_equal(other, emulate(frame, item["aug"].numpy(), b"", other_hw))
        else:
            assert len(raw) == RESULT_BYTES + n0 and np.array_equal(root, want_other)


def test_hostile_estimates_under_the_sanitizers(check_exe):
    """NaN, +-inf, +-1e300, -1e9, all key-points on each side of the frame, one point, have = 0, 1 x 1 and 4096 x 1 frames, records no
    geometry would produce: every case ends with a valid or whole-frame crop and a finite positive k_value, no read leaves a frame
    of exactly H * W * 3 bytes (ASan), no float -> int cast or index overflows (UBSan); track_update clears ``have``."""
    exe, _ = check_exe
    r = subprocess.run([exe, "hostile"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "hostile failures 0", r.stdout
    status = {(w[1], int(w[3])): int(w[5]) for w in (ln.split() for ln in lines) if w[0] == "case"}
    both = nv.TRACK_NO_ESTIMATE | nv.TRACK_BAD_BOX
    for name in ("nan", "plus_inf", "minus_inf", "all_plus_1e300", "all_minus_1e300", "all_minus_1e9", "left", "right", "above", "below",
                 "one_point", "frame_1x4096_nan"):
        assert status[(name, 0)] == both, name
    for name in ("have_0", "have_0_nan_state", "frame_1x1_have_0", "frame_4096x1_have_0"):
        assert all(status[(name, m)] == nv.TRACK_NO_ESTIMATE for m in range(3)), name
    for name in ("good", "one_plus_1e300", "one_minus_1e300", "one_minus_1e9", "frame_1x1", "frame_4096x1"):
        assert status[(name, 0)] in (0, both), name
    assert status[("good", 0)] == 0 and status[("one_point", 1)] == 0
    have = {w[1]: int(w[3]) for w in (ln.split() for ln in lines) if w[0] == "update"}
    assert have["good"] == 1 and have["two_inside_of_two_wanted"] == 1
    for name in ("nan", "inf", "z_zero", "z_negative", "all_outside", "one_inside_of_two_wanted"):
        assert have[name] == 0, name
    assert any(ln.startswith("wrong_records") and int(ln.split()[1]) > 4000 for ln in lines)


def _prepare_args(**over):
    """Arguments of hrp_track_prepare that pass every host check (the pointers are never followed on the host)."""
    a = dict(frames=64, kp2d=64, have=64, K=64, B=1, H=480, W=640, nkp=7, out_root=64, h0=256, w0=256, out_other=None, h1=0, w1=0,
             extend=(C.c_double * 2)(0.2, 0.13), mode=nv.TRACK_BBOX_EXTENDED, K_root=64, K_other=64, k_values=64, geom=64, stream=None)
    a.update(over)
    return list(a.values())


def _update_args(**over):
    a = dict(xyz=64, K=64, B=1, nkp=7, W=640, H=480, min_inside=1, kp2d=64, have=64, out=64, status=64, stream=None)
    a.update(over)
    return list(a.values())


def test_entry_points_refuse_bad_arguments_without_a_gpu(check_exe):
    lib = nv.lib()
    bad = [dict(frames=None), dict(kp2d=None), dict(have=None), dict(K=None), dict(out_root=None), dict(extend=None), dict(K_root=None),
           dict(K_other=None), dict(k_values=None), dict(geom=None), dict(nkp=0), dict(nkp=33), dict(nkp=-1), dict(H=4097), dict(W=4097),
           dict(H=0), dict(W=0), dict(h0=4097), dict(w0=4097), dict(h0=0), dict(out_other=64, h1=4097, w1=128),
           dict(out_other=64, h1=128, w1=0), dict(mode=3), dict(mode=-1), dict(B=0)]
    for over in bad:
        assert lib.hrp_track_prepare(*_prepare_args(**over)) == -1, over
        assert b"track_prepare" in lib.hrp_last_error(), over
    bad = [dict(xyz=None), dict(K=None), dict(kp2d=None), dict(have=None), dict(out=None), dict(status=None), dict(nkp=0), dict(nkp=33),
           dict(W=4097), dict(H=4097), dict(W=0), dict(H=0), dict(B=0)]
    for over in bad:
        assert lib.hrp_track_update(*_update_args(**over)) == -1, over
        assert b"track_update" in lib.hrp_last_error(), over
    with pytest.raises(nv.HrpError):
        nv.call("hrp_track_prepare", *_prepare_args(nkp=33))
    exe, _ = check_exe
    size = int(subprocess.run([exe, "sizeof"], stdout=subprocess.PIPE, text=True, check=True).stdout)
    assert size == C.sizeof(nv.TrackGeom) == np.dtype(nv.TrackGeom).itemsize == 112


def test_tracker_refuses_a_cpu_device():
    from hrpe_amd.lib.core.tracker import PoseTracker
    K = np.array([[615.0, 0, 320], [0, 615, 240], [0, 0, 1]])
    with pytest.raises(nv.HrpError):
        PoseTracker(lambda *a: None, None, K, (480, 640), device="cpu")
    assert nv.TRACK_NO_ESTIMATE == 1 and nv.TRACK_BAD_BOX == 2 and nv.TRACK_LOST_OUT == 4
    assert torch.float64 == PoseTracker.STATE_DTYPE
