"""The device JPEG decode (csrc/jpeg.hip) on the GPU: every supported case of tests/golden/golden_jpeg.npz in one call against
Pillow's recorded decode, repeated and under graph replay, and DreamDataset(device_decode=True) through to_device.  Valid files
only: damaged streams are decoded on the CPU (tests/test_jpeg_host.py)."""
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
    return datas, [J.parse_header(d) for d in datas]


def test_all_cases_in_one_call_equal_pillow(files):
    """Twelve files of seven sizes, three sub-samplings, default and optimised tables, with and without restart intervals."""
    datas, hdrs = files
    frames, status = J.decode_batch(datas, hdrs, DEV)
    assert status.dtype == torch.int32 and status.is_cuda and list(J.check_status(status)) == [0] * len(NAMES)
    for n, f in zip(NAMES, frames):
        got = f.cpu()
        assert got.dtype == torch.uint8 and got.shape == want(n).shape
        assert torch.equal(got, want(n)), f"{n}: {int((got != want(n)).sum())} of {got.numel()} bytes differ"


def test_second_call_and_graph_replay_give_the_same_bytes(files):
    datas, hdrs = files
    b = J.Batch(datas, np.stack(hdrs), DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b.launch()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first = b.flat.clone()
    assert torch.equal(first, torch.cat([want(n).reshape(-1) for n in NAMES]).to(DEV))
    for t in (b.flat, b.planes, b.coef):
        t.fill_(7)
    b.status.fill_(-1)
    b.launch()
    torch.cuda.synchronize()
    assert torch.equal(b.flat, first) and not b.status.any()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.launch()
    for t in (b.flat, b.planes, b.coef):
        t.fill_(9)
    b.status.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(b.flat, first) and not b.status.any()


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), path
    else:
        assert type(a) is type(b) and a == b, path


def test_dataset_device_decode_equals_the_host_form(tmp_path):
    base = str(tmp_path / "panda_synth_test_dr")
    paths = dream_scene.write_scene(base, frames=dream_scene.FRAMES[:2])
    ds = D.DreamDataset(base, device_decode=True, process_truncation=True, occlu_p=1.0)
    random.seed(11)
    np.random.seed(11)
    items = [ds[i % 2] for i in range(4)]
    assert all("frame" not in it and len(it["jpeg"]) and it["jpeg_host"] == b"" for it in items)
    batch = torch.utils.data.default_collate(items)
    out_dev = ds.to_device(batch, DEV)
    torch.cuda.synchronize()
    host = dict(batch)
    for k in ("jpeg", "jpeg_hdr", "jpeg_host"):
        del host[k]
    host["frame"] = out_dev["images_original"].permute(0, 2, 3, 1).cpu().contiguous()
    out_host = ds.to_device(host, DEV)
    torch.cuda.synchronize()
    assert out_dev["root"]["images"].dtype == torch.uint8 and out_dev["root"]["images"].shape == (4, 3, 256, 256)
    assert torch.equal(out_dev["root"]["images"], out_host["root"]["images"])
    assert torch.equal(out_dev["other"]["images"], out_host["other"]["images"])
    _same(out_dev, out_host)
    datas = [open(paths[i % 2], "rb").read() for i in range(4)]
    frames, status = J.decode_batch(datas, [J.parse_header(d) for d in datas], DEV)
    assert not J.check_status(status).any()
    assert out_dev["images_original"].shape == (4, 3, 480, 640)
    assert torch.equal(out_dev["images_original"], torch.stack(frames).permute(0, 3, 1, 2))
    # a status list defers the check
    st = []
    ds.to_device(batch, DEV, jpeg_status=st)
    assert len(st) == 1 and not J.check_status(st[0]).any()


def test_batch_with_a_progressive_file_takes_the_host_frame_for_it():
    names = ["optimize_40x56_420", "progressive_40x56", "rst_rows1_40x56_420"]
    enc = [D._Encoded(file_of(n)) for n in names]
    assert [len(e.jpeg) > 0 for e in enc] == [True, False, True] and len(enc[1].host) == 40 * 56 * 3
    frames, status = D.decode_frames([e.jpeg for e in enc], np.stack([e.hdr for e in enc]), [e.host for e in enc], DEV)
    torch.cuda.synchronize()
    assert frames.shape == (3, 40, 56, 3) and status.shape == (2,) and not J.check_status(status).any()
    for i, n in enumerate(names):
        assert torch.equal(frames[i].cpu(), want(n)), n
