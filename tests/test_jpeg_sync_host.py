"""CPU-only checks of the many-lanes-per-segment entropy stage of the device JPEG decode (hrp_jpeg_decode_sync): the decoder
core's jpeg_sync_subseq under tests/jpeg_sync_host_check.cpp, which runs the kernel's schedule lane by lane against the serial
decoder on every fixture case and on the damaged corpus; the host-side argument checks of the entry point; the short / long
split of jpeg.Batch."""
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
from hrpe_amd.lib.dataset import jpeg as J  # noqa: E402
from test_jpeg_host import DAMAGED, GOLD, NAMES, RESTART, file_of  # noqa: E402,F401

STUFFED_AT_16 = {"odd_23x37_420", "optimize_40x56_420", "q100_sat_48x64_420", "q50_48x64_420", "tall_33x17_420"}


def parsed(name):
    data = file_of(name)
    recs = np.array([J.record(J.parse_header(data))])
    return data, recs, J.split_segments(np.frombuffer(data, dtype=np.uint8), recs)


@pytest.fixture(scope="module")
def sync_check(tmp_path_factory):
    """Build tests/jpeg_sync_host_check.cpp with the host compiler (no sanitizer), run it once, return its exit status, its
    output, the per-case lines and the last line as dicts."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("jpeg_sync_host")
    exe = str(td / "jpeg_sync_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "jpeg_sync_host_check.cpp"), "-o", exe], check=True)
    blob = [np.int32(len(NAMES)).tobytes()]
    for name in NAMES:
        data, recs, segs = parsed(name)
        rgb = np.ascontiguousarray(GOLD[name + "/rgb"])
        blob += [np.int32(name in DAMAGED).tobytes(), recs.tobytes(), np.int32(len(segs)).tobytes(), segs.tobytes(),
                 np.int64(len(data)).tobytes(), data, np.int64(rgb.size).tobytes(), rgb.tobytes()]
    cases = td / "cases.bin"
    cases.write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    lines = r.stdout.strip().splitlines()
    per_case = {}
    for ln in lines:
        w = ln.split()
        if len(w) == 8 and w[0] == "case" and w[2] == "subseq":
            per_case[NAMES[int(w[1])]] = {"subseq": int(w[3]), "rounds": int(w[5]), "wrong": int(w[7])}
    last = [w for w in lines[-1].split() if w != "|"]
    totals = {}
    section = ""
    for k, v in zip(last[0::2], last[1::2]):
        if k in ("valid", "order", "damaged", "looped"):
            section = k
        totals[k if k == section else section + "_" + k] = int(v)
    return r.returncode, r.stdout, per_case, totals


def test_every_case_equals_the_serial_decoder_and_pillow(sync_check):
    """S = 16, 64, 4096 (a single lane): coefficients equal jpeg_decode_segment's, status 0, the frame equal to Pillow's."""
    rc, out, per_case, n = sync_check
    assert rc == 0, out
    assert n["valid"] == 3 * len(NAMES) and n["valid_mismatch"] == 0, out
    assert set(per_case) == set(NAMES), out
    assert min(c["subseq"] for c in per_case.values()) >= 9 and per_case["rows_96x128_420"]["subseq"] >= 424, out


def test_result_depends_neither_on_the_guess_nor_on_the_lane_order(sync_check):
    """Three guessed start states, lanes ascending and descending; and the rounds did run: some case had a lane whose first exit
    state was wrong and needed two or more rounds."""
    rc, out, per_case, n = sync_check
    assert n["order"] == 6 * len(NAMES) and n["order_differ"] == 0, out
    assert n["looped"] >= 1, out
    assert any(c["wrong"] > 0 and c["rounds"] >= 2 for c in per_case.values()), out


def test_fixtures_have_a_stuffed_zero_on_a_boundary():
    """At S = 16 some sub-sequence of some segment begins on the 00 of an FF 00 (counted from the files' bytes)."""
    hits = {}
    for name in NAMES:
        data, _, segs = parsed(name)
        for s in segs:
            off, ln = int(s["off"]), int(s["len"])
            for lo in range(16, ln, 16):
                if data[off + lo] == 0 and data[off + lo - 1] == 0xFF:
                    hits[name] = hits.get(name, 0) + 1
    assert sum(hits.values()) >= 1, hits
    assert set(hits) == STUFFED_AT_16 and sum(hits.values()) == 6, hits


def test_damaged_streams_equal_the_serial_decoder(sync_check):
    """Truncation at every 97th length and 200 single-byte changes of three cases, at S = 16 and 128, and a marker 0 .. 9 bytes
    behind the last MCU inside the segment: coefficients, status and frame as jpeg_decode_segment leaves them on the same bytes,
    every guard (the scratch's included) intact."""
    rc, out, per_case, n = sync_check
    assert rc == 0, out
    assert n["damaged"] >= 2 * (3 * 200 + 3 * 10 + 3 * 10) and n["damaged_guard"] == 0 and n["damaged_differ"] == 0, out
    assert n["damaged_serial"] >= 1, out               # the reader-history case did occur and took jpeg_segment_status


def _sync_args(**over):
    """Arguments of hrp_jpeg_decode_sync that pass every host check (the pointers are never followed on the host)."""
    nbytes, S, nlong = 4096, 64, 1
    a = dict(images=64, B=1, short=64, nshort=1, long=64, nlong=nlong, S=S, bytes=64, nbytes=nbytes, coef=64, ncoef=64 * 6,
             planes=64, nplanes=64 * 6, frames=64, nframes=3 * 64, scratch=64, nscratch=None, status=64, stream=None)
    a.update(over)
    if a["nscratch"] is None:
        a["nscratch"] = nv.lib().hrp_jpeg_sync_scratch_bytes(a["nbytes"], a["nlong"], a["S"])
    return [a[k] for k in ("images", "B", "short", "nshort", "long", "nlong", "S", "bytes", "nbytes", "coef", "ncoef", "planes",
                           "nplanes", "frames", "nframes", "scratch", "nscratch", "status", "stream")]


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = nv.lib()
    assert lib.hrp_jpeg_sync_scratch_bytes(4096, 1, 64) == 32 * (4096 // 64 + 2 + 1)
    assert lib.hrp_jpeg_sync_scratch_bytes(4096, 1, 48) == 0
    bad = [dict(S=48), dict(S=8), dict(S=8192), dict(S=0), dict(nscratch=32), dict(scratch=72), dict(scratch=None), dict(images=None),
           dict(bytes=None), dict(coef=None), dict(planes=None), dict(frames=None), dict(status=None), dict(nshort=0, nlong=0),
           dict(short=None), dict(long=None), dict(nshort=-1), dict(B=0)]
    for over in bad:
        if "S" in over:
            over.setdefault("nscratch", 1 << 20)
        assert lib.hrp_jpeg_decode_sync(*_sync_args(**over)) == -1, over
        assert lib.hrp_last_error()
    assert lib.hrp_jpeg_decode_sync(*_sync_args(nscratch=lib.hrp_jpeg_sync_scratch_bytes(4096, 1, 64) - 1)) == -1
    assert b"scratch" in lib.hrp_last_error()
    with pytest.raises(nv.HrpError):
        nv.call("hrp_jpeg_decode_sync", *_sync_args(S=48, nscratch=1 << 20))


def test_batch_sync_on_a_cpu_device_raises():
    data = file_of("rows_96x128_420")
    hdr = J.parse_header(data)
    for entropy in ("segment", "sync"):
        with pytest.raises(nv.HrpError):
            J.decode_batch([data], [hdr], torch.device("cpu"), entropy=entropy)
    with pytest.raises(nv.HrpError, match="not a GPU"):
        J.Batch([data], hdr[None], torch.device("cpu"), entropy="sync")
    with pytest.raises(nv.HrpError):
        J.Batch([data], hdr[None], torch.device("cpu"), entropy="huffman")
    with pytest.raises(nv.HrpError):
        J.Batch([data], hdr[None], torch.device("cpu"), entropy="sync", subseq_bytes=48)


def test_split_long_short_on_the_restart_fixtures():
    """min_subseq chosen between the shortest and the longest segment of each restart fixture: some segments on each side, every
    segment on exactly one, both lists in ascending order."""
    for name in RESTART:
        data, recs, segs = parsed(name)
        S = 16
        spans = -(-segs["len"] // S)
        assert spans.min() < spans.max(), name
        m = int(spans.min()) + 1
        short, long_ = J.split_long(segs, S, m)
        assert len(short) and len(long_) and len(short) + len(long_) == len(segs)
        assert (-(-short["len"] // S) < m).all() and (-(-long_["len"] // S) >= m).all()
        assert sorted(list(short["off"]) + list(long_["off"])) == list(segs["off"])
        assert (np.diff(long_["off"]) > 0).all() and (np.diff(short["off"]) > 0).all()
        everything, none = J.split_long(segs, S, 1)[1], J.split_long(segs, S, 1 << 30)[1]
        assert len(everything) == len(segs) and len(none) == 0
    assert J.SUBSEQ_BYTES in (32, 64, 128, 256) and J.MIN_SUBSEQ >= 1
    assert C.sizeof(C.c_size_t) == 8
