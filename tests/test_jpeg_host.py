"""CPU-only checks of the device JPEG decode's host side and of its decoder core (csrc/jpeg_core.h, compiled for the host):
parse_header against Pillow on every case of tests/golden/golden_jpeg.npz, and tests/jpeg_host_check.cpp - the same functions
the kernels call - on every supported case (bytes equal to Pillow's decode) and on a seeded corpus of damaged streams."""
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.dataset import jpeg as J  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "golden_jpeg.npz"))
NAMES = [str(n) for n in GOLD["names"]]
FALLBACK = [str(n) for n in GOLD["fallback"]]
DAMAGED = ("odd_23x37_422", "optimize_40x56_420", "rst_blocks2_40x56_420")   # 4:2:2, optimised tables, restart intervals
SAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}
RESTART = {"rst_blocks2_40x56_420": 2, "rst_rows1_40x56_420": 4}            # rows=1: one row of ceil(56 / 16) MCUs


def file_of(name):
    return GOLD[name + "/file"].tobytes()


def test_ctypes_mirrors_match_the_header(tmp_path):
    """sizeof and a late field's offset of the three JPEG structs, from a C program compiled against include/hrp.h."""
    import ctypes as C
    (tmp_path / "s.c").write_text("""#include <stdio.h>
#include <stddef.h>
#include "hrp.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %d\\n", sizeof(hrp_jpeg_huff), sizeof(hrp_jpeg_image), sizeof(hrp_jpeg_segment),
         offsetof(hrp_jpeg_image, ac), offsetof(hrp_jpeg_segment, mcu0), HRP_JPEG_WARN_TRAILING);
  return 0;
}""")
    exe = str(tmp_path / "s")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [C.sizeof(nv.JpegHuff), C.sizeof(nv.JpegImage), C.sizeof(nv.JpegSegment), nv.JpegImage.ac.offset,
                   nv.JpegSegment.mcu0.offset, nv.JPEG_WARN_TRAILING]
    assert J.HDR_BYTES == C.sizeof(nv.JpegImage) and J.SEG_DTYPE.itemsize == C.sizeof(nv.JpegSegment)


def test_fixture_lists_the_cases_of_the_issue():
    assert len(NAMES) == 12 and set(FALLBACK) == {"progressive_40x56", "gray_40x56", "narrow_20x3_420"}
    assert set(DAMAGED) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_parse_header_matches_pillow(name):
    from PIL import Image
    data = file_of(name)
    hdr = J.parse_header(data)
    assert hdr is not None and hdr.dtype == np.uint8 and hdr.shape == (J.HDR_BYTES,)
    r = J.record(hdr)
    im = Image.open(io.BytesIO(data))
    h, w, _ = GOLD[name + "/rgb"].shape
    assert (int(r["width"]), int(r["height"])) == im.size == (w, h)
    assert (int(r["hsamp"]), int(r["vsamp"])) == SAMPLING[name.rsplit("_", 1)[1]]
    layer = im.layer                                   # (component id, h, v, quantisation table) per component
    assert [(c[1], c[2]) for c in layer] == [(int(r["hsamp"]), int(r["vsamp"])), (1, 1), (1, 1)]
    assert [c[3] for c in layer] == [int(v) for v in r["comp_tq"][:3]]
    for tq, table in im.quantization.items():          # Pillow gives the tables in natural order, as the record holds them
        assert list(table) == [int(v) for v in r["quant"][tq]], f"quantisation table {tq}"
    assert int(r["restart_interval"]) == RESTART.get(name, 0)
    assert data[int(r["scan_off"]) - 10:int(r["scan_off"]) - 9] == b"\x03" and int(r["scan_off"]) + int(r["scan_len"]) == len(data)
    for kind in ("dc", "ac"):                          # complete, prefix-free code lengths and as many symbols
        for t in r[kind]:
            counts = t["counts"].astype(np.int64)
            assert 0 < counts.sum() <= 256
            assert (counts * 2.0 ** -np.arange(1, 17)).sum() <= 1.0
    # a collated stack gives the records back
    both = J.record(np.stack([hdr, hdr]))
    assert both.shape == (2,) and both[1] == r


@pytest.mark.parametrize("name", FALLBACK)
def test_parse_header_refuses_what_the_device_does_not_decode(name):
    assert J.parse_header(file_of(name)) is None


def test_parse_header_checks_every_length():
    data = file_of("odd_23x37_420")
    scan = int(J.record(J.parse_header(data))["scan_off"])
    for n in range(0, scan):                           # every truncation inside the header is refused, none raises
        assert J.parse_header(data[:n]) is None
    assert J.parse_header(data[:scan]) is not None
    assert J.parse_header(b"") is None and J.parse_header(b"\xff\xd8\xff") is None


def test_split_segments_follows_the_restart_markers():
    for name, ri in RESTART.items():
        data = file_of(name)
        recs = np.array([J.record(J.parse_header(data))])
        segs = J.split_segments(np.frombuffer(data, dtype=np.uint8), recs)
        assert len(segs) == -(-(3 * 4) // ri) and list(segs["mcu0"]) == list(range(0, 12, ri))
        for k, s in enumerate(segs):
            end = int(s["off"]) + int(s["len"])
            assert data[end] == 0xFF and data[end + 1] == (0xD0 + k % 8 if k + 1 < len(segs) else 0xD9)
        assert int(recs[0]["scan_off"]) + int(recs[0]["scan_len"]) == len(data) - 2
    bad = bytearray(file_of("rst_rows1_40x56_420"))
    first = int(J.split_segments(np.frombuffer(bytes(bad), dtype=np.uint8), np.array([J.record(J.parse_header(bytes(bad)))]))[0]["len"])
    hdr = J.record(J.parse_header(bytes(bad)))
    bad[int(hdr["scan_off"]) + first + 1] = 0xD5       # RST0 -> RST5
    with pytest.raises(nv.HrpError):
        J.split_segments(np.frombuffer(bytes(bad), dtype=np.uint8), np.array([hdr]))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """Build tests/jpeg_host_check.cpp with the host compiler (no sanitizer), run it once on every case, return its last line
    as a dict."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("jpeg_host")
    exe = str(td / "jpeg_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "jpeg_host_check.cpp"), "-o", exe], check=True)
    blob = [np.int32(len(NAMES)).tobytes()]
    for name in NAMES:
        data = file_of(name)
        recs = np.array([J.record(J.parse_header(data))])
        segs = J.split_segments(np.frombuffer(data, dtype=np.uint8), recs)
        rgb = np.ascontiguousarray(GOLD[name + "/rgb"])
        blob += [np.int32(name in DAMAGED).tobytes(), recs.tobytes(), np.int32(len(segs)).tobytes(), segs.tobytes(),
                 np.int64(len(data)).tobytes(), data, np.int64(rgb.size).tobytes(), rgb.tobytes()]
    cases = td / "cases.bin"
    cases.write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    last = r.stdout.strip().splitlines()[-1].replace("|", " ").split()
    return r.returncode, r.stdout, dict(zip(last[0::2], (int(v) for v in last[1::2])))


def test_host_decode_of_every_case_equals_pillow(host_check):
    rc, out, n = host_check
    assert rc == 0, out
    assert n["valid"] == len(NAMES) and n["mismatch"] == 0, out


def test_damaged_streams_return_with_guards_intact(host_check):
    rc, out, n = host_check
    assert rc == 0, out
    assert n["damaged"] >= 3 * 200 + 3 * 10 and n["guard"] == 0, out
    assert n["differ"] > n["damaged"] // 2, out        # the corpus does damage what is decoded


def test_damaged_streams_that_decode_differently_report_it(host_check):
    """Status non-zero whenever the frame differs from the fixture's.

    Measured (g++, the same with -fsanitize=address,undefined): 653 damaged runs (53 truncations, 600 single-byte
    changes), 652 decode to other bytes, none of them under status 0.  The decoder's own errors report every truncation and
    211 of the 599 byte changes that alter the frame; 147 more end off their padding bits (HRP_JPEG_WARN_TRAILING).  The other 241 change magnitude
    bits, or turn one Huffman code into another such that the scan still ends on its last bit: they are well-formed scans of
    another image, which no decoder tells from the original.  What reports them is HRP_JPEG_ERR_CHECKSUM: the header record
    carries the Adler-32 that parse_header took of the bytes it read, and one byte changed always changes it."""
    rc, out, n = host_check
    assert n["silent"] == 0, out
    assert n["checksum_only"] + n["trailing_only"] < n["differ"], out      # the decoder's own errors still fire


def test_header_record_is_tied_to_its_bytes():
    """scan_sum is zlib's Adler-32 from the first entropy-coded byte to the end of the file; Batch refuses a record whose
    lengths are not its file's."""
    import zlib
    data = file_of("rows_96x128_420")
    hdr = J.parse_header(data)
    r = J.record(hdr)
    assert int(r["scan_sum"]) == zlib.adler32(data[int(r["scan_off"]):]) and int(r["sum_len"]) == len(data) - int(r["scan_off"])
    import torch
    with pytest.raises(nv.HrpError):
        J.Batch([data + b"\x00"], hdr[None], torch.device("cpu"))
def test_dataset_items_carry_the_file_instead_of_the_frame(tmp_path):
    """DreamDataset(device_decode=True): same draws and geometry as the host form, the file's bytes and header in place of the
    frame; a file that parse_header refuses travels as Pillow's decode."""
    import random
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dream_scene
    from PIL import Image
    from hrpe_amd.lib.dataset import dream as D
    base = str(tmp_path / "panda_synth_test_dr")
    paths = dream_scene.write_scene(base, frames=dream_scene.FRAMES[:2])
    Image.open(paths[1]).save(paths[1], quality=92, progressive=True)
    items = {}
    for dd in (False, True):
        ds = D.DreamDataset(base, device_decode=dd, occlu_p=1.0)
        random.seed(3)
        np.random.seed(3)
        items[dd] = [ds[0], ds[1]]
    for a, b in zip(items[False], items[True]):
        assert set(a) - {"frame"} == set(b) - {"jpeg", "jpeg_hdr", "jpeg_host"} and "frame" not in b
        assert torch.equal(a["aug"], b["aug"]) and a["noise"] == b["noise"] and torch.equal(a["root"]["K"], b["root"]["K"])
    dev, host = items[True]
    assert dev["jpeg"] == open(paths[0], "rb").read() and dev["jpeg_host"] == b""
    r = J.record(dev["jpeg_hdr"].numpy())
    assert (int(r["width"]), int(r["height"])) == (640, 480) and dev["jpeg_hdr"].shape == (J.HDR_BYTES,)
    assert host["jpeg"] == b"" and host["jpeg_host"] == items[False][1]["frame"].numpy().tobytes()
    batch = torch.utils.data.default_collate(items[True])
    assert batch["jpeg_hdr"].shape == (2, J.HDR_BYTES) and isinstance(batch["jpeg"], list)
    with pytest.raises(nv.HrpError):
        D.to_device(batch, device="cpu")
