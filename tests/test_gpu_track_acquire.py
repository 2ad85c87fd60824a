"""Tracker acquisition on the GPU (hrp_track_seed, PoseTracker.seed / acquire / step with acquire_every): the kernel against the
float64 numpy rule of tests/track_seed_oracle.py (the cases of the host sanitizer run), a closed loop with a stub detector, graph
capture of the seed launch, one step with seg_mask_inference.detect as the detector without a host synchronisation, and the launch
sequence of step with and without a detector."""
import ctypes as C
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.core.tracker import PoseTracker  # noqa: E402
import track_seed_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FX = FY = 615.0
CX, CY = 320.0, 240.0
K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])
ROBOT = types.SimpleNamespace(nkp=7)


def xyz_of(kp2d, depth=1.25):
    """Camera-frame points (float32) that project onto kp2d [.., 2] with K."""
    kp2d = np.asarray(kp2d, np.float64)
    z = depth + 0.05 * np.arange(kp2d.shape[-2])
    xyz = np.stack([(kp2d[..., 0] - CX) / FX * z, (kp2d[..., 1] - CY) / FY * z, np.broadcast_to(z, kp2d.shape[:-1])], -1)
    return torch.from_numpy(xyz.astype(np.float32))


def stub_outputs(xyz):
    B = xyz.shape[0]
    z = lambda *s: torch.zeros(B, *s, device=xyz.device)   # noqa: E731
    return z(8), z(6), z(3), z(2), z(1), z(7, 3), z(7, 3), xyz


def seed_call(cs):
    """hrp_track_seed on a batch of oracle cases that share everything but det / ms / mask / state / have"""
    c0, B, nkp = cs[0], len(cs), len(cs[0]["det"])
    det = torch.from_numpy(np.stack([c["det"] for c in cs]).astype(np.float32)).to(DEV)
    mask = None if c0["mask"] is None else torch.from_numpy(np.stack([c["mask"] for c in cs])).to(DEV)
    ms = None if c0["ms"] is None else torch.from_numpy(np.stack([c["ms"] for c in cs])).to(DEV)
    state = torch.from_numpy(np.stack([c["state"] for c in cs]).astype(np.float64)).to(DEV)
    have = torch.tensor([c["have"] for c in cs], dtype=torch.int32, device=DEV)
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    hm, wm = (0, 0) if mask is None else mask.shape[1:]
    nv.call("hrp_track_seed", det.data_ptr(), B, nkp, (C.c_double * 2)(*c0["inv"]), None if mask is None else mask.data_ptr(), hm, wm,
            float(c0["min_prob"]), None if ms is None else ms.data_ptr(), float(c0["min_peak"]), int(c0["min_inside"]), int(c0["force"]),
            c0["W"], c0["H"], state.data_ptr(), have.data_ptr(), status.data_ptr(), None)
    torch.cuda.synchronize()
    return status.cpu().numpy(), have.cpu().numpy(), state.cpu().numpy()


def test_seed_kernel_equals_numpy():
    cases = O.cases(np.random.default_rng(11)) + O.cases(np.random.default_rng(13), nkp=32, W=4096, H=4096, hm=64, wm=64)[:8]
    seen = set()
    for n, c in enumerate(cases):
        if not np.isfinite(c["inv"]).all():
            with pytest.raises(nv.HrpError, match="track_seed"):
                seed_call([c])
            continue
        st, have, state = seed_call([c])
        w_st, w_have, w_state = O.seed(**c)
        assert (int(st[0]), int(have[0])) == (w_st, w_have), n
        assert np.array_equal(state[0].view(np.uint64), np.ascontiguousarray(w_state, np.float64).view(np.uint64)), n
        seen.add(w_st)
    assert seen == {O.SKIPPED, O.TAKEN, O.REFUSED}
    # one launch over 70 streams (two workgroups) that differ in det / state / have, with a mask and ms
    rng = np.random.default_rng(5)
    base = O.cases(rng)[0]
    mask = rng.uniform(0, 1, (70, 240, 320)).astype(np.float32)
    batch = []
    for b in range(70):
        c = dict(base, det=(rng.uniform(-20, 340, (7, 2)) * [1.0, 0.75]).astype(np.float32), mask=mask[b], min_prob=0.3, min_inside=3,
                 ms=np.stack([rng.normal(size=7), rng.uniform(1, 6, 7)], 1).astype(np.float32), min_peak=0.25,
                 state=rng.normal(size=(7, 2)), have=int(b % 3 == 0))
        batch.append(c)
    st, have, state = seed_call(batch)
    want = [O.seed(**c) for c in batch]
    assert st.tolist() == [w[0] for w in want] and have.tolist() == [w[1] for w in want]
    assert np.array_equal(state, np.stack([w[2] for w in want]))
    assert {O.SKIPPED, O.TAKEN, O.REFUSED} == set(st.tolist())


def _loop_script():
    """4 frames x 2 streams.  Detections (detector pixels, scale 0.5) and the model's predictions (frame pixels):
    stream 0: seeded at frame 0, tracked, a NaN prediction at frame 1 loses it, the detection of frame 2 recovers it;
    stream 1: its detection of frame 0 is refused (one key-point is NaN) and its predictions of frames 0 and 1 are NaN, so it
    crops the whole frame until the detection of frame 2 is taken."""
    rng = np.random.default_rng(3)
    unit = rng.uniform(-1, 1, (7, 2))
    det = np.zeros((4, 2, 7, 2), np.float32)
    pred = np.zeros((4, 2, 7, 2))
    for t in range(4):
        det[t, 0] = (np.array([150, 110]) + 5 * t) + unit * [40, 35]
        det[t, 1] = (np.array([210, 150]) - 4 * t) + unit * [30, 45]
        pred[t, 0] = (np.array([310, 230]) + 9 * t) + unit * [85, 70]
        pred[t, 1] = (np.array([400, 290]) - 7 * t) + unit * [60, 95]
    det[0, 1, 4, 0] = np.nan
    xyz = torch.stack([xyz_of(pred[t]) for t in range(4)])
    xyz[1, 0, 2, 1] = float("nan")
    xyz[0, 1, 0, 0] = float("nan")
    xyz[1, 1, 5, 2] = float("nan")
    return torch.from_numpy(det), xyz


def test_closed_loop_with_a_stub_detector():
    det, xyz = _loop_script()
    det, xyz = det.to(DEV), xyz.to(DEV)
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (4, 2, 480, 640, 3), dtype=torch.uint8, generator=g).to(DEV)
    t = [0]
    seen = []

    def detector(img):
        seen.append((t[0], tuple(img.shape), img.dtype, img.is_contiguous()))
        assert torch.equal(img, frames[t[0]].permute(0, 3, 1, 2))
        return det[t[0]], None, None
    trk = PoseTracker(lambda reg, root, k, Kc: stub_outputs(xyz[t[0]]), ROBOT, K, (480, 640), streams=2, rootnet_resize_hw=(128, 128),
                      other_resize_hw=(96, 96), device=DEV, detector=detector, detector_scale=0.5, acquire_every=2)
    ref = PoseTracker(None, ROBOT, K, (480, 640), streams=2, rootnet_resize_hw=(128, 128), other_resize_hw=(96, 96), device=DEV)
    log = []
    for t[0] in range(4):
        res = trk.step(frames[t[0]])
        log.append(dict(seed=trk.seed_status.clone(), geom=trk.geom.clone(), status=res.status.clone(), have=trk.have.clone(),
                        root=trk.root_images.clone(), kp2d=trk.kp2d.clone()))
    torch.cuda.synchronize()
    assert [s[0] for s in seen] == [0, 2] and seen[0][1:] == ((2, 3, 480, 640), torch.uint8, True)
    seeds = [f["seed"].cpu().tolist() for f in log]
    assert seeds[0] == [nv.SEED_TAKEN, nv.SEED_REFUSED] and seeds[1] == seeds[0]           # frame 1 runs no detection
    assert seeds[2] == [nv.SEED_TAKEN, nv.SEED_TAKEN] and seeds[3] == seeds[2]
    status = [f["status"].cpu().tolist() for f in log]
    whole = nv.TRACK_NO_ESTIMATE
    assert status[0] == [0, whole | nv.TRACK_LOST_OUT]                                     # seeded; no estimate and a NaN prediction
    assert status[1] == [nv.TRACK_LOST_OUT, whole | nv.TRACK_LOST_OUT]                     # stream 0 tracked from frame 0's prediction, then lost
    assert status[2] == [0, 0] and status[3] == [0, 0]                                     # both recovered at the scheduled detection
    assert [f["have"].cpu().tolist() for f in log] == [[1, 0], [0, 0], [1, 1], [1, 1]]
    # the crops of the frames with a detection are the crops of a tracker reset to detection * (1 / scale), bit for bit
    for tt, streams in ((0, [0]), (2, [0, 1])):
        ref.reset(None)
        ref.reset(det[tt, streams].double().cpu().numpy() * 2.0, streams=streams)
        ref.prepare(frames[tt])
        for b in streams:
            assert torch.equal(ref.geom[b], log[tt]["geom"][b]) and torch.equal(ref.root_images[b], log[tt]["root"][b]), (tt, b)
        if tt == 0:
            assert torch.equal(ref.geom[1], log[0]["geom"][1])                             # the refused stream took the whole frame
    # a stream with an estimate skips a detection unless forced; the thresholds reach the kernel
    t[0] = 3
    assert trk.acquire(frames[3]).cpu().tolist() == [nv.SEED_SKIPPED, nv.SEED_SKIPPED]
    before = trk.kp2d.clone()
    assert trk.acquire(frames[3], force=True, min_inside=8).cpu().tolist() == [nv.SEED_REFUSED, nv.SEED_REFUSED]
    assert torch.equal(trk.kp2d, before) and trk.have.cpu().tolist() == [1, 1]
    assert trk.acquire(frames[3], force=True).cpu().tolist() == [nv.SEED_TAKEN, nv.SEED_TAKEN]
    assert torch.equal(trk.kp2d, det[3].double() * 2.0)
    mask = torch.zeros(2, 1, 240, 320, device=DEV)
    mask[1] = 1.0
    ms = torch.ones(2, 7, 2, device=DEV)
    assert trk.seed(det[2], mask, ms, force=True).cpu().tolist() == [nv.SEED_REFUSED, nv.SEED_TAKEN]
    assert trk.seed(det[2], mask[:, 0], ms * 4, force=True, min_peak=0.5).cpu().tolist() == [nv.SEED_REFUSED, nv.SEED_REFUSED]
    for bad in (lambda: trk.seed(det[2].cpu()), lambda: trk.seed(det[2, :, :6]), lambda: trk.seed(det[2], mask[:1]),
                lambda: trk.seed(det[2], ms=ms[:, :6]), lambda: ref.acquire(frames[0]),
                lambda: PoseTracker(None, ROBOT, K, (480, 640), device=DEV, acquire_every=2),
                lambda: PoseTracker(None, ROBOT, K, (480, 640), device=DEV, detector=detector, detector_scale=0.0)):
        with pytest.raises(nv.HrpError):
            bad()


def test_graph_replay_of_the_seed_launch_equals_eager():
    rng = np.random.default_rng(8)
    sets = []
    for i in range(3):
        det = torch.from_numpy((rng.uniform(-30, 350, (3, 7, 2)) * [1.0, 0.75]).astype(np.float32)).to(DEV)
        mask = torch.from_numpy(rng.uniform(0, 1, (3, 1, 240, 320)).astype(np.float32)).to(DEV)
        ms = torch.from_numpy(np.stack([rng.normal(size=(3, 7)), rng.uniform(1, 5, (3, 7))], -1).astype(np.float32)).to(DEV)
        sets.append((det, mask, ms))
    kw = dict(min_inside=3, min_prob=0.3, min_peak=0.25)

    def new():
        trk = PoseTracker(None, ROBOT, K, (480, 640), streams=3, device=DEV)
        trk.reset(np.full((1, 7, 2), 9.0), streams=[2])
        return trk
    trk, eager = new(), []
    for det, mask, ms in sets:
        trk.seed(det, mask, ms, **kw)
        eager.append((trk.seed_status.clone(), trk.kp2d.clone(), trk.have.clone()))
    assert len({tuple(e[0].cpu().tolist()) for e in eager}) > 1 and eager[0][0][2].item() == nv.SEED_SKIPPED
    trk = new()
    bufs = [torch.zeros_like(t) for t in sets[0]]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        trk.seed(*bufs, min_inside=8)                                     # warm-up on the capture stream (refused: the state is untouched)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        trk.seed(*bufs, **kw)
    for (det, mask, ms), want in zip(sets, eager):
        for b, src in zip(bufs, (det, mask, ms)):
            b.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((trk.seed_status, trk.kp2d, trk.have), want))


def test_step_with_the_network_detector_does_not_synchronise():
    """B = 1, seg_mask_inference(...).detect as the detector on 128 x 192 frames: after the plan's warm-up calls (build, graph
    capture) a step under torch.cuda.set_sync_debug_mode("warn") raises no warning."""
    from hrpe_amd.lib.models.ctrnet.mask_inference import seg_mask_inference
    torch.manual_seed(4)
    H, W = 128, 192
    net = seg_mask_inference((150.0, 150.0, 96.0, 64.0), "azure", image_hw=(H, W), allow_random_init=True).to(DEV)
    Ks = np.array([[150.0, 0, 96], [0, 150.0, 64], [0, 0, 1]])
    xyz = torch.tensor([[[0.05 * i - 0.15, 0.03 * i - 0.1, 1.0 + 0.02 * i] for i in range(7)]], device=DEV)
    trk = PoseTracker(lambda reg, root, k, Kc: stub_outputs(xyz), ROBOT, Ks, (H, W), streams=1, rootnet_resize_hw=(64, 64),
                      other_resize_hw=(64, 64), device=DEV, detector=net.detect, detector_scale=net.args.scale, acquire_every=1)
    frames = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=DEV)
    for _ in range(4):
        trk.reset(None)
        trk.step(frames)
    torch.cuda.synchronize()
    first = trk.seed_status.clone()
    trk.reset(None)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            res = trk.step(frames)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert not [str(w.message) for w in rec if "synchron" in str(w.message).lower()], [str(w.message) for w in rec]
    assert torch.equal(trk.seed_status, first) and int(first[0]) in (nv.SEED_TAKEN, nv.SEED_REFUSED)
    assert res.kp2d_original.shape == (1, 7, 2) and trk.have.cpu().tolist() == [1]
    kp, prob, ms = net.detect(frames.permute(0, 3, 1, 2).contiguous())
    assert kp.shape == (1, 7, 2) and prob.shape == (1, 1, H // 2, W // 2) and ms.shape == (1, 7, 2)


def test_launch_sequence_of_step():
    """Without a detector step issues exactly prepare and update; with one, the seed launch in front on the scheduled frames."""
    xyz = xyz_of(np.array([[[300.0 + 10 * i, 200.0 + 8 * i] for i in range(7)]])).to(DEV)
    frames = torch.randint(0, 256, (1, 480, 640, 3), dtype=torch.uint8, device=DEV)
    det = torch.full((1, 7, 2), 100.0, device=DEV)
    names = []

    def hook(name, args, launch):
        names.append(name)
        launch()
    model = lambda reg, root, k, Kc: stub_outputs(xyz)   # noqa: E731
    plain = PoseTracker(model, ROBOT, K, (480, 640), device=DEV)
    sched = PoseTracker(model, ROBOT, K, (480, 640), device=DEV, detector=lambda img: (det, None, None), acquire_every=3)
    off = PoseTracker(model, ROBOT, K, (480, 640), device=DEV, detector=lambda img: (det, None, None))
    nv.set_profile_hook(hook)
    try:
        for _ in range(2):
            plain.step(frames)
        assert names == ["hrp_track_prepare", "hrp_track_update"] * 2
        del names[:]
        for _ in range(2):
            off.step(frames)
        assert names == ["hrp_track_prepare", "hrp_track_update"] * 2
        del names[:]
        for _ in range(4):
            sched.step(frames)
        step = ["hrp_track_prepare", "hrp_track_update"]
        assert names == ["hrp_track_seed"] + step * 3 + ["hrp_track_seed"] + step
    finally:
        nv.set_profile_hook(None)
    torch.cuda.synchronize()
