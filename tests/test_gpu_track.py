"""PoseTracker (lib/core/tracker.py, csrc/track.hip) on the GPU against the existing host path of the DREAM loader fed the tracker's
own read-back float64 state (tests/track_oracle.py): prepare, update, the closed loop with a stub model, graph capture, no host
synchronisation, and one end-to-end step with the HRNet-W32 pair."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.core.tracker import PoseTracker  # noqa: E402
from hrpe_amd.lib.dataset import dream as D  # noqa: E402
import dream_scene  # noqa: E402
import track_oracle as O  # noqa: E402
from test_dream_host import CASES, GOLD, need_frame, scene  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VIEW_PAIRS = [((128, 128), (128, 128)), ((256, 256), (256, 256)), ((216, 216), (128, 128))]
K_SCENE = np.array([[dream_scene.FX, 0, dream_scene.CX], [0, dream_scene.FY, dream_scene.CY], [0, 0, 1.0]])
ROBOT = types.SimpleNamespace(nkp=7)


def frame_of(base, i):
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(os.path.join(base, "%06d.rgb.jpg" % i)), dtype=np.uint8))


def seeds_of(base, idx):
    ds = D.DreamDataset(base, color_jitter=False, rgb_augmentation=False, occlusion_augmentation=False)
    return np.stack([np.asarray(ds[i]["keypoints_2d_original"], np.float64) for i in idx])


def xyz_of(kp2d, depth=1.25):
    """Camera-frame points (float32) that project onto kp2d [.., 2] with the scene's K."""
    kp2d = np.asarray(kp2d, np.float64)
    z = depth + 0.05 * np.arange(kp2d.shape[-2])
    xyz = np.stack([(kp2d[..., 0] - dream_scene.CX) / dream_scene.FX * z, (kp2d[..., 1] - dream_scene.CY) / dream_scene.FY * z,
                    np.broadcast_to(z, kp2d.shape[:-1])], -1)
    return torch.from_numpy(xyz.astype(np.float32))


def stub_outputs(xyz):
    """A model output tuple in RootNetwithRegInt's order with ``xyz`` as xyz_fk."""
    B = xyz.shape[0]
    z = lambda *s: torch.zeros(B, *s, device=xyz.device)   # noqa: E731
    return z(8), z(6), z(3), z(2), z(1), z(7, 3), z(7, 3), xyz


def check_against_host_path(trk, frames, kp2d, have, mode="extended", where=""):
    """The tracker's buffers after prepare(frames) against the host path run on the state (kp2d, have) read back BEFORE it."""
    torch.cuda.synchronize()
    recs = [O.tracker_record(kp2d[b], int(have[b]), K_SCENE, trk.W, trk.H, trk.root_hw, trk.other_hw, mode) for b in range(trk.B)]
    want_root, want_other = O.host_images(frames, recs, trk.root_hw, trk.other_hw)
    assert torch.equal(trk.root_images, want_root), where
    assert torch.equal(trk.reg_images, want_other), where
    geom = O.geom_array(trk.geom)
    K_root, K_other, k = trk.root_K.cpu().numpy(), trk.other_K.cpu().numpy(), trk.k_values.cpu().numpy()
    for b, rec in enumerate(recs):
        O.check_record(geom[b], K_root[b], K_other[b], float(k[b]), rec, mode, (where, b))
    return recs


@pytest.mark.parametrize("frames_idx", [(0, 1, 2, 3), (4,)])
@pytest.mark.parametrize("pair", VIEW_PAIRS)
def test_prepare_equals_the_host_path(scene, frames_idx, pair):  # noqa: F811
    frames = torch.stack([frame_of(scene, i) for i in frames_idx]).to(DEV)
    B, H, W, _ = frames.shape
    seeds = seeds_of(scene, frames_idx)
    for mode, kw in (("extended", {}), ("origin", dict(use_extended_bbox=False, use_origin_bbox=True)),
                     ("strict", dict(use_extended_bbox=False))):
        trk = PoseTracker(None, ROBOT, K_SCENE, (H, W), streams=B, rootnet_resize_hw=pair[0], other_resize_hw=pair[1], device=DEV, **kw)
        trk.reset(seeds)
        kp2d, have = trk.kp2d.cpu().numpy(), trk.have.cpu().numpy()
        assert np.array_equal(kp2d, seeds) and have.all()                 # float64 kept bit for bit
        out = trk.prepare(frames)
        recs = check_against_host_path(trk, frames, kp2d, have, mode, (frames_idx, pair, mode))
        assert all(r["status"] == 0 for r in recs) and not trk.status.any()
        assert (out["root_images"] is out["reg_images"]) == (pair[0] == pair[1])
        assert out["root_K"].shape == (B, 3, 3) and out["k_values"].shape == (B,)
    if pair[0] == (216, 216) and 3 in frames_idx:
        assert O.geom_array(trk.geom)[3]["side"] == 216                   # the copy path (side == out)


def test_prepare_equals_the_reference_bytes(scene):  # noqa: F811
    case = CASES["off"]
    need_frame(scene, case)
    frames = frame_of(scene, 0)[None].to(DEV)
    trk = PoseTracker(None, ROBOT, K_SCENE, (480, 640), rootnet_resize_hw=(128, 128), other_resize_hw=(128, 128), device=DEV)
    trk.reset(seeds_of(scene, [0]))
    out = trk.prepare(frames)
    torch.cuda.synchronize()
    assert np.array_equal(out["root_images"][0].cpu().numpy(), GOLD["off/root/images"])
    assert np.allclose(out["root_K"][0].cpu().numpy(), GOLD["off/root/K"], atol=O.ATOL, rtol=O.RTOL)


def test_update_equals_float64_numpy():
    """B = 5: a good estimate, one with a NaN, one with a negative Z, one with all points outside, one with exactly min_inside points
    inside.  Both sides are float64 arithmetic on the same float32 inputs."""
    min_inside = 2
    rng = np.random.default_rng(7)
    inside = np.stack([rng.uniform(20, 620, (5, 7)), rng.uniform(20, 460, (5, 7))], -1)
    inside[3] += 2000.0                                                  # all outside
    inside[4, min_inside:] -= 3000.0                                     # exactly min_inside inside
    xyz = xyz_of(inside)
    xyz[1, 4, 1] = float("nan")
    xyz[2, 5, 2] = -1.5
    trk = PoseTracker(None, ROBOT, K_SCENE, (480, 640), streams=5, min_inside=min_inside, device=DEV)
    got2d = trk.update(xyz.to(DEV))
    torch.cuda.synchronize()
    x = xyz.numpy().astype(np.float64)
    Kf = K_SCENE.astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        want = np.stack([Kf[0, 0] * x[..., 0] / x[..., 2] + Kf[0, 2], Kf[1, 1] * x[..., 1] / x[..., 2] + Kf[1, 2]], -1)
    n_in = ((want[..., 0] >= 0) & (want[..., 0] < 640) & (want[..., 1] >= 0) & (want[..., 1] < 480)).sum(1)
    assert list(n_in) == [7, 6, n_in[2], 0, min_inside]
    want_have = np.array([1, 0, 0, 0, 1], np.int32)
    np.testing.assert_allclose(trk.kp2d.cpu().numpy(), want, rtol=1e-9, atol=0, equal_nan=True)
    np.testing.assert_allclose(got2d.cpu().numpy(), want.astype(np.float32), rtol=1e-6, atol=0, equal_nan=True)
    assert np.array_equal(trk.have.cpu().numpy(), want_have)
    assert np.array_equal(trk.status.cpu().numpy(), np.where(want_have == 1, 0, nv.TRACK_LOST_OUT))
    # one fewer inside than min_inside is refused
    trk2 = PoseTracker(None, ROBOT, K_SCENE, (480, 640), streams=5, min_inside=min_inside + 1, device=DEV)
    trk2.update(xyz.to(DEV))
    assert trk2.have.cpu().tolist() == [1, 0, 0, 0, 0]


def _sequence(fail):
    """Prescribed predictions of 4 frames x 2 streams: the boxes move, shrink under the 150 x 120 minimum and touch the border;
    fail: stream 1's prediction of frame 1 holds a NaN."""
    rng = np.random.default_rng(11)
    unit = rng.uniform(-1, 1, (7, 2))
    boxes = {0: [((330, 250), (120, 140)), ((420, 200), (30, 25)), ((60, 240), (110, 150)), ((300, 260), (90, 80))],
             1: [((200, 300), (100, 90)), ((250, 280), (80, 70)), ((580, 400), (130, 120)), ((320, 240), (20, 15))]}
    xyz = torch.stack([torch.stack([xyz_of(np.array(c) + np.array(s) * unit) for c, s in boxes[b]]) for b in (0, 1)], 1)   # [4, 2, 7, 3]
    if fail:
        xyz[1, 1, 2, 0] = float("nan")
    return xyz


def _run_loop(scene, fail):  # noqa: F811
    xyz = _sequence(fail).to(DEV)
    t = [0]
    trk = PoseTracker(lambda reg, root, k, K: stub_outputs(xyz[t[0]]), ROBOT, K_SCENE, (480, 640), streams=2,
                      rootnet_resize_hw=(128, 128), other_resize_hw=(96, 96), device=DEV)
    trk.reset(seeds_of(scene, [0, 1]))
    log = []
    for t[0] in range(4):
        frames = torch.stack([frame_of(scene, t[0] % 4), frame_of(scene, (t[0] + 1) % 4)]).to(DEV)
        kp2d, have = trk.kp2d.cpu().numpy(), trk.have.cpu().numpy()
        res = trk.step(frames)
        recs = check_against_host_path(trk, frames, kp2d, have, where=("frame", t[0], "fail", fail))
        log.append(dict(recs=recs, kp_before=kp2d, root=trk.root_images.clone(), reg=trk.reg_images.clone(), geom=trk.geom.clone(),
                        status=res.status.clone(), k=res.k_values.clone(), kp2d=trk.kp2d.clone(), have=trk.have.clone(),
                        kp2d_original=res.kp2d_original.clone()))
    torch.cuda.synchronize()
    return log


def test_closed_loop_with_a_stub_model(scene):  # noqa: F811
    """After every frame the next crop equals the host path run on the read-back state; a NaN prediction costs stream 1 one
    whole-frame crop and nothing else; stream 0 never notices."""
    bad, good = _run_loop(scene, True), _run_loop(scene, False)
    crops = [tuple(f["recs"][b]["crop"] for b in (0, 1)) for f in bad]
    assert len({c[0] for c in crops}) == 4                                # stream 0's box moves every frame
    assert any(c[0][0] == 0 for c in crops)                               # touches the border
    widths = [(c[0][2] - c[0][0], np.ptp(f["kp_before"][0, :, 0])) for c, f in zip(crops, bad)]
    assert any(kw * 1.6 + 2 < 150 and cw > kw * 1.6 + 140 for cw, kw in widths), widths       # under 150 wide: grown by 75 a side
    status = torch.stack([f["status"] for f in bad]).cpu().numpy()        # after each frame's update
    assert status[:, 0].tolist() == [0, 0, 0, 0]
    assert status[:, 1].tolist() == [0, nv.TRACK_LOST_OUT, nv.TRACK_NO_ESTIMATE, 0]
    assert [int(f["have"][1]) for f in bad] == [1, 0, 1, 1]
    assert bad[2]["recs"][1]["crop"] == (0, 0, 640, 480) and bad[2]["recs"][1]["status"] == nv.TRACK_NO_ESTIMATE
    assert bad[3]["recs"][1]["status"] == 0 and bad[3]["recs"][1]["crop"] == good[3]["recs"][1]["crop"]        # recovered
    assert not torch.equal(bad[2]["root"][1], good[2]["root"][1])
    for f, g in zip(bad, good):                                           # stream 0: byte-identical to the run without the failure
        for k in ("root", "reg", "geom", "status", "k", "kp2d", "have", "kp2d_original"):      # kp_before is numpy, covered by kp2d
            assert torch.equal(f[k][0], g[k][0]), k


def _graph_stub(base, direction, p):
    """A few tensor operations standing in for the network: the prediction depends on the crop it was given."""
    shift = p["root_images"].float().mean(dim=(1, 2, 3)) * 1e-4 + p["k_values"] * 1e-6
    return base + shift[:, None, None] * direction


def test_graph_capture_of_prepare_and_update(scene):  # noqa: F811
    batches = [torch.stack([frame_of(scene, i) for i in idx]).to(DEV) for idx in ((0, 1), (2, 3))]
    seeds = seeds_of(scene, [0, 1])
    base = xyz_of(seeds).to(DEV)
    fb = torch.empty_like(batches[0])
    direction = torch.tensor([1.0, -1.0, 0.0], device=DEV)

    def new():
        trk = PoseTracker(None, ROBOT, K_SCENE, (480, 640), streams=2, rootnet_resize_hw=(128, 128), other_resize_hw=(96, 96), device=DEV)
        trk.reset(seeds)
        return trk

    def body(trk):
        trk.update(_graph_stub(base, direction, trk.prepare(fb)))

    def snapshot(trk):
        return [t.clone() for t in (trk.root_images, trk.reg_images, trk.root_K, trk.other_K, trk.k_values, trk.geom, trk.kp2d, trk.have,
                                    trk.status, trk.kp2d_original)]

    def eager():
        trk, snaps = new(), []
        for b in batches:
            fb.copy_(b)
            body(trk)
            snaps.append(snapshot(trk))
        return snaps

    first, second = eager(), eager()
    for a, b in zip(first, second):
        assert all(torch.equal(x, y) for x, y in zip(a, b))               # the second eager run equals the first
    assert not torch.equal(first[0][0], first[1][0]) and not torch.equal(first[0][6], first[1][6])
    trk = new()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    fb.copy_(batches[0])
    with torch.cuda.stream(s):
        body(trk)                                                         # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body(trk)                                                         # one linear chain: prepare -> tensor ops -> update
    trk.reset(seeds)
    for b, want in zip(batches, first):
        fb.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        got = snapshot(trk)
        assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_prepare_and_update_do_not_synchronise(scene):  # noqa: F811
    frames = torch.stack([frame_of(scene, 0), frame_of(scene, 1)]).to(DEV)
    seeds = seeds_of(scene, [0, 1])
    xyz = xyz_of(seeds).to(DEV)
    trk = PoseTracker(None, ROBOT, K_SCENE, (480, 640), streams=2, device=DEV)
    trk.reset(seeds)
    trk.update(xyz)
    trk.prepare(frames)                                                   # warmed up
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            trk.prepare(frames)
            trk.update(xyz)
            trk.update((None, xyz))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert trk.have.cpu().tolist() == [1, 1]


def test_tracker_refuses_what_it_cannot_take(scene):  # noqa: F811
    trk = PoseTracker(None, ROBOT, K_SCENE, (480, 640), streams=2, device=DEV)
    frames = torch.stack([frame_of(scene, 0), frame_of(scene, 1)])
    with pytest.raises(nv.HrpError):
        trk.prepare(frames)                                               # CPU frames
    with pytest.raises(nv.HrpError):
        trk.prepare(frames.to(DEV)[:, :400])                              # not frame_hw
    with pytest.raises(nv.HrpError):
        trk.prepare(frames.to(DEV).float())
    with pytest.raises(nv.HrpError):
        trk.update(torch.zeros(2, 7, 3))                                  # CPU prediction
    with pytest.raises(nv.HrpError):
        trk.update(torch.zeros(2, 6, 3, device=DEV))
    with pytest.raises(nv.HrpError):
        trk.reset(np.zeros((2, 6, 2)))
    trk.reset(np.full((1, 7, 2), 5.0), streams=[1])
    assert trk.have.cpu().tolist() == [0, 1] and float(trk.kp2d[1, 0, 0]) == 5.0 and float(trk.kp2d[0, 0, 0]) == 0.0


def test_end_to_end_with_the_network(scene):  # noqa: F811
    """HRNet-W32 pair, B = 2, 256 x 256, seeded from the fixture's ``size256`` case (frame 3).  The images the model receives equal
    DreamDataset.to_device's for that case's frame, views and key-points byte for byte - with the dataset's augmentation draws
    switched off: the fixture case itself draws colour jitter, an occlusion and three enhancements, which a tracker on live frames
    has no counterpart for; the crop geometry does not depend on them."""
    from test_gpu_dream import _model
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    case = CASES["size256"]
    need_frame(scene, case)
    ds = D.DreamDataset(scene, color_jitter=False, rgb_augmentation=False, occlusion_augmentation=False,
                        rootnet_resize_hw=tuple(case["kw"]["rootnet_resize_hw"]), other_resize_hw=tuple(case["kw"]["other_resize_hw"]))
    item = ds[case["frame"]]
    want = ds.to_device(torch.utils.data.default_collate([item, item]), DEV)
    frames = want["images_original"].permute(0, 2, 3, 1).contiguous()
    seeds = np.stack([np.asarray(item["keypoints_2d_original"], np.float64)] * 2)
    model = _model().to(DEV)
    robot = URDFRobot("panda")
    seen = []

    model.register_forward_pre_hook(lambda m, args: seen.append((args[0].clone(), args[1].clone())))

    def run(feed):
        trk = PoseTracker(model, robot, K_SCENE, (480, 640), streams=2, device=DEV)
        trk.reset(seeds)
        res = trk.step(feed)
        torch.cuda.synchronize()
        return trk, res

    trk, res = run(frames)
    assert torch.equal(seen[0][0], want["other"]["images"]) and torch.equal(seen[0][1], want["root"]["images"])
    assert not model.training
    for name, t in res._asdict().items():
        assert torch.isfinite(t.float()).all(), name
    assert res.kp3d.shape == (2, 7, 3) and res.kp2d_original.shape == (2, 7, 2) and res.pose.shape[0] == 2
    # the state after step is update applied to the returned kp3d
    ref = PoseTracker(None, robot, K_SCENE, (480, 640), streams=2, device=DEV)
    ref.update(res.kp3d)
    assert torch.equal(ref.kp2d, trk.kp2d) and torch.equal(ref.have, trk.have)
    assert torch.equal(ref.kp2d_original, res.kp2d_original)
    snap = [t.clone() for t in res]
    state = trk.kp2d.clone()
    trk2, res2 = run(frames)                                              # a second tracker from the same seed: bit-identical
    assert all(torch.equal(a, b) for a, b in zip(snap, res2)) and torch.equal(state, trk2.kp2d)
    # one call on the JPEG files' bytes gives the same tensors as the decoded-frame call, where the device decoder equals Pillow
    data = open(os.path.join(scene, "%06d.rgb.jpg" % case["frame"]), "rb").read()
    trk3 = PoseTracker(model, robot, K_SCENE, (480, 640), streams=2, device=DEV)
    decoded = trk3.decode([data, data])
    torch.cuda.synchronize()
    assert torch.equal(decoded, frames)
    trk3.reset(seeds)
    res3 = trk3.step([data, data])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(snap, res3)) and torch.equal(state, trk3.kp2d)
