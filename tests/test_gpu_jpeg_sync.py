"""The many-lanes-per-segment entropy stage of the device JPEG decode (hrp_jpeg_decode_sync, jpeg.Batch(entropy="sync")) on the
GPU: frames against Pillow's recorded bytes, frames and coefficients against the one-lane-per-segment path on the same files,
repeated and under graph replay with every buffer - the scratch included - overwritten in between, and through DreamDataset.
Valid files only: damaged streams are decoded on the CPU (tests/test_jpeg_sync_host.py)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd.lib.dataset import dream as D  # noqa: E402
from hrpe_amd.lib.dataset import jpeg as J  # noqa: E402
import dream_scene  # noqa: E402
from test_jpeg_host import GOLD, NAMES, file_of  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def want(name):
    return torch.from_numpy(GOLD[name + "/rgb"])


@pytest.fixture(scope="module")
def files():
    datas = [file_of(n) for n in NAMES]
    return datas, np.stack([J.parse_header(d) for d in datas])


@pytest.fixture(scope="module")
def segment_path(files):
    """The one-lane-per-segment decode of the fixture files: computed once, read by the tests below."""
    b = J.Batch(files[0], files[1], DEV)
    b.launch()
    assert not J.check_status(b.status).any()
    return b.coef.clone(), b.flat.clone()


@pytest.mark.parametrize("kw", [dict(subseq_bytes=16, min_subseq=2), dict()], ids=["s16", "defaults"])
def test_all_cases_in_one_call_equal_pillow_and_the_segment_path(files, segment_path, kw):
    datas, hdrs = files
    b = J.Batch(datas, hdrs, DEV, entropy="sync", **kw)
    assert len(b.short) + len(b.long) == len(b.segments)
    if kw:
        assert len(b.long) >= len(NAMES)                       # every file, restart intervals too
    b.launch()
    assert list(J.check_status(b.status)) == [0] * len(NAMES)
    for n, f in zip(NAMES, b.frames()):
        got = f.cpu()
        assert got.shape == want(n).shape and torch.equal(got, want(n)), f"{n}: {int((got != want(n)).sum())} of {got.numel()} bytes differ"
    assert torch.equal(b.coef, segment_path[0]) and torch.equal(b.flat, segment_path[1])
    r = b.rounds()
    assert len(r) == len(b.long) and (r >= 1).all()
    if kw:
        assert r.max() >= 2                                    # the rounds did run


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    """Two frames of the procedural scene as DreamDataset reads them, 640 x 480 and a 400 x 300 re-encoding, no restart markers."""
    import io
    from PIL import Image
    base = str(tmp_path_factory.mktemp("scene") / "panda_synth_test_dr")
    paths = dream_scene.write_scene(base, frames=dream_scene.FRAMES[:2])
    big = open(paths[0], "rb").read()
    buf = io.BytesIO()
    Image.open(paths[1]).resize((400, 300)).save(buf, format="JPEG", quality=92)
    return base, paths, [big, buf.getvalue()]


@pytest.mark.parametrize("kw", [dict(subseq_bytes=16), dict()], ids=["s16", "defaults"])
def test_scene_frames_equal_the_segment_path(scene_files, kw):
    """At 16 bytes the large frame has thousands of sub-sequences for 512 lanes: the lanes stride."""
    datas = scene_files[2]
    hdrs = np.stack([J.parse_header(d) for d in datas])
    ref = J.Batch(datas, hdrs, DEV)
    ref.launch()
    assert not J.check_status(ref.status).any()
    assert [tuple(f.shape) for f in ref.frames()] == [(480, 640, 3), (300, 400, 3)]
    b = J.Batch(datas, hdrs, DEV, entropy="sync", **kw)
    assert len(b.long) == 2 and len(b.short) == 0
    if kw:
        assert -(-int(b.long["len"][0]) // 16) > 4 * 512
    b.launch()
    assert not J.check_status(b.status).any()
    assert torch.equal(b.coef, ref.coef) and torch.equal(b.flat, ref.flat)


def test_mixed_batch_through_decode_frames():
    """An optimised-table file for the workgroup kernel, a progressive one decoded on the host, a restart file whose segments stay
    on the one-lane kernel."""
    names = ["optimize_40x56_420", "progressive_40x56", "rst_rows1_40x56_420"]
    enc = [D._Encoded(file_of(n)) for n in names]
    recs = J.record(np.stack([e.hdr for e in enc]))[[0, 2]].copy()
    sizes = [len(enc[0].jpeg), len(enc[2].jpeg)]
    recs["scan_off"] += [0, sizes[0]]
    segs = J.split_segments(np.frombuffer(enc[0].jpeg + enc[2].jpeg, dtype=np.uint8), recs)
    spans = -(-segs["len"] // 16)
    m = int(spans[1:].max()) + 1
    short, long_ = J.split_long(segs, 16, m)
    assert len(long_) == 1 and int(long_["image"][0]) == 0 and len(short) == len(segs) - 1
    frames, status = D.decode_frames([e.jpeg for e in enc], np.stack([e.hdr for e in enc]), [e.host for e in enc], DEV, entropy="sync",
                                     subseq_bytes=16, min_subseq=m)
    torch.cuda.synchronize()
    assert frames.shape == (3, 40, 56, 3) and status.shape == (2,) and not J.check_status(status).any()
    for i, n in enumerate(names):
        assert torch.equal(frames[i].cpu(), want(n)), n


def test_second_call_and_graph_replay_give_the_same_bytes(files, segment_path):
    datas, hdrs = files
    b = J.Batch(datas, hdrs, DEV, entropy="sync", subseq_bytes=16, min_subseq=2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b.launch()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(b.flat, segment_path[1]) and torch.equal(b.coef, segment_path[0]) and not b.status.any()

    def junk(v):
        for t in (b.flat, b.planes, b.coef, b.scratch):
            t.fill_(v)
        b.status.fill_(-1)
    junk(7)
    b.launch()
    torch.cuda.synchronize()
    assert torch.equal(b.flat, segment_path[1]) and torch.equal(b.coef, segment_path[0]) and not b.status.any()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.launch()
    junk(9)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(b.flat, segment_path[1]) and torch.equal(b.coef, segment_path[0]) and not b.status.any()


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), path
    else:
        assert type(a) is type(b) and a == b, path


def test_dataset_with_the_sync_stage_equals_the_default(scene_files):
    base = scene_files[0]
    ds = D.DreamDataset(base, device_decode=True, process_truncation=True, occlu_p=1.0)
    ds_sync = D.DreamDataset(base, device_decode=True, process_truncation=True, occlu_p=1.0, jpeg_entropy="sync")
    assert ds.jpeg_entropy == "segment" and ds_sync.jpeg_entropy == "sync"
    random.seed(11)
    np.random.seed(11)
    batch = torch.utils.data.default_collate([ds[i % 2] for i in range(4)])
    out = ds.to_device(batch, DEV)
    out_sync = ds_sync.to_device(batch, DEV)
    torch.cuda.synchronize()
    assert out_sync["images_original"].shape == (4, 3, 480, 640)
    _same(out_sync, out)
