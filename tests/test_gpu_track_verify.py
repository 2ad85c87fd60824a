"""Tracker verification on the GPU (hrp_track_verify, PoseTracker.verify / acquire with min_support / min_coverage / min_iou): the
kernel against the float64 numpy rule of tests/track_verify_oracle.py (the cases of the host sanitizer run), a closed loop in which
a stream that locked onto the wrong crop is dropped and reseeded, the launch sequence, graph capture of verify + seed, a step
without a host synchronisation, and the silhouette path with a box mesh."""
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
import track_verify_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FX = FY = 615.0
CX, CY = 320.0, 240.0
K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])
ROBOT = types.SimpleNamespace(nkp=7, robot_type="panda")          # (panda: the default bones are the serial chain)


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


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def verify_call(cs, alpha_shift=0):
    """hrp_track_verify on a batch of oracle cases that share everything but state / have / mask / alpha.  alpha_shift: the
    silhouette starts that many floats behind a 16-byte boundary (the mask starts on one)."""
    c0, B, nkp = cs[0], len(cs), len(cs[0]["state"])
    hm, wm = c0["mask"].shape
    state = torch.from_numpy(np.stack([c["state"] for c in cs])).to(DEV)
    have = torch.tensor([c["have"] for c in cs], dtype=torch.int32, device=DEV)
    mask = torch.from_numpy(np.stack([c["mask"] for c in cs])).to(DEV)
    alpha = None
    if c0["alpha"] is not None:
        buf = torch.zeros(B * hm * wm + 8, device=DEV)
        alpha = buf[alpha_shift:alpha_shift + B * hm * wm]
        alpha.copy_(torch.from_numpy(np.stack([c["alpha"] for c in cs]).reshape(-1)))
        assert alpha.data_ptr() % 16 == 4 * alpha_shift and mask.data_ptr() % 16 == 0
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((B, 4), -1, dtype=torch.int32, device=DEV)
    sums = torch.full((B, 3), -1.0, dtype=torch.float64, device=DEV)
    d = nv.TrackVerifyDesc()
    d.state_kp2d, d.state_have, d.mask, d.alpha = state.data_ptr(), have.data_ptr(), mask.data_ptr(), None if alpha is None else alpha.data_ptr()
    d.verify_status, d.counts, d.sums = status.data_ptr(), counts.data_ptr(), sums.data_ptr()
    d.B, d.nkp, d.hm, d.wm, d.nb, d.samples, d.min_fg, d.min_samples = B, nkp, hm, wm, len(c0["bones"]), c0["samples"], c0["min_fg"], c0["min_samples"]
    for i, (a, b) in enumerate(c0["bones"]):
        d.bones[i][0], d.bones[i][1] = int(a), int(b)
    (d.scale[0], d.scale[1]), (d.extend_ratio[0], d.extend_ratio[1]) = c0["scale"], c0["extend_ratio"]
    d.min_support, d.min_coverage, d.min_iou, d.min_prob = c0["min_support"], c0["min_coverage"], c0["min_iou"], c0["min_prob"]
    nv.call("hrp_track_verify", C.byref(d), None)
    torch.cuda.synchronize()
    return status, have, counts, sums, state


def held_to_the_oracle(cs, got, what):
    status, have, counts, sums, state = [t.cpu().numpy() for t in got]
    seen = set()
    for b, c in enumerate(cs):
        hm, wm = c["mask"].shape
        w_st, w_have, w_counts, w_sums = O.verify(**O.call_args(c))
        assert (int(status[b]), int(have[b]), counts[b].tolist()) == (w_st, w_have, w_counts.tolist()), (what, b, status[b], counts[b], w_st, w_counts)
        assert np.array_equal(state[b].view(np.uint64), c["state"].view(np.uint64)), (what, b)          # never written
        assert O.sums_ok(sums[b], w_sums, hm * wm, c["exact"]), (what, b, sums[b], w_sums)
        seen.add(w_st)
    return seen


def shared_key(c):
    return (len(c["state"]), c["mask"].shape, tuple(map(tuple, c["bones"])), c["alpha"] is not None) + \
        tuple(c[k] for k in ("samples", "scale", "extend_ratio", "min_prob", "min_fg", "min_samples", "min_support", "min_coverage", "min_iou"))


def test_verify_kernel_equals_numpy():
    cases = O.cases()
    seen = set()
    for n, c in enumerate(cases):                                    # B = 1
        got = verify_call([c])
        seen |= held_to_the_oracle([c], got, n)
        if n % 7 == 0 or c["mask"].shape == (17, 33):                # two runs are bit-equal
            again = verify_call([c])
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again)), n
    assert seen == O.ALL_OUTCOMES, sorted(seen)
    # B = 3, streams that differ in state / have / maps, mixed outcomes in one launch; 17 x 33 maps start off a 16-byte boundary
    groups = {}
    for c in cases:
        groups.setdefault(shared_key(c), []).append(c)
    batches = [g[i:i + 3] for g in groups.values() for i in range(0, len(g) - 2, 3)]
    mixed, shapes = set(), set()
    for n, cs in enumerate(batches):
        got = verify_call(cs)
        st = held_to_the_oracle(cs, got, ("batch", n))
        again = verify_call(cs)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again)), n
        mixed |= {len(st) > 1}
        shapes.add(cs[0]["mask"].shape)
    assert True in mixed and {(17, 33), (60, 80)} <= shapes and len(batches) >= 5
    # a silhouette whose alignment differs from the mask's (the scalar walk): the same counts, sums within the same bound
    with_alpha = [cs for cs in batches if cs[0]["alpha"] is not None][:3] + [[c] for c in cases if c["alpha"] is not None][:12]
    assert len(with_alpha) >= 10
    for n, cs in enumerate(with_alpha):
        for shift in (1, 3):
            held_to_the_oracle(cs, verify_call(cs, alpha_shift=shift), ("shift", shift, n))


# ---- closed loop -------------------------------------------------------------------------------------------------------------
def _loop_pieces():
    """Two streams on 640 x 480 frames, detector at half resolution.  The detector sees the robot in the bottom-right quarter (a
    blob and the key-points in it); the model's prediction for stream 0 lies on the blob, for stream 1 in the top-left quarter."""
    rng = np.random.default_rng(3)
    unit = rng.uniform(-1, 1, (7, 2))
    pred = np.stack([np.array([480.0, 360.0]) + unit * [50, 40], np.array([160.0, 120.0]) + unit * [50, 40]])
    det = np.stack([(np.array([480.0, 360.0]) + unit * [45, 35]) * 0.5, (np.array([470.0, 350.0]) + unit * [45, 35]) * 0.5]).astype(np.float32)
    blob = O.ellipse(240, 320, 240.0, 180.0, 60.0, 50.0).astype(np.float32)
    mask = torch.from_numpy(np.stack([blob, blob])[:, None]).to(DEV)
    return xyz_of(pred).to(DEV), torch.from_numpy(det).to(DEV), mask


def _run_loop(frames, **kw):
    xyz, det, mask = _loop_pieces()
    empty = [False]
    trk = PoseTracker(lambda reg, root, k, Kc: stub_outputs(xyz), ROBOT, K, (480, 640), streams=2, rootnet_resize_hw=(128, 128),
                      other_resize_hw=(96, 96), device=DEV, detector=lambda img: (det, torch.zeros_like(mask) if empty[0] else mask, None),
                      detector_scale=0.5, acquire_every=2, **kw)
    log = []
    for t in range(4):
        trk.step(frames[t])
        log.append(dict(seed=trk.seed_status.cpu().tolist(), verify=trk.verify_status.cpu().tolist(), have=trk.have.cpu().tolist(),
                        geom=[nv.TrackGeom.from_buffer_copy(bytes(trk.geom[b].cpu().numpy())) for b in range(2)], kp2d=trk.kp2d.clone()))
    return trk, log, det, empty


def test_closed_loop_drops_and_reseeds_a_drifted_stream():
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (4, 2, 480, 640, 3), dtype=torch.uint8, generator=g).to(DEV)
    # today's behaviour: stream 1 keeps cropping the top-left quarter, the scheduled detection of frame 2 is skipped
    plain, plog, det, _ = _run_loop(frames)
    assert plog[0]["seed"] == [nv.SEED_TAKEN, nv.SEED_TAKEN] and plog[2]["seed"] == [nv.SEED_SKIPPED, nv.SEED_SKIPPED]
    for t in (1, 2, 3):
        g1 = plog[t]["geom"][1]
        assert g1.status == 0 and g1.crop_x1 <= 320 and g1.crop_y1 <= 240, (t, g1.crop_x1, g1.crop_y1)
    assert plog[2]["verify"] == [0, 0]                                                       # never launched
    # with min_support the stream is dropped and takes the detection in the same acquire
    trk, log, det, empty = _run_loop(frames, min_support=0.5)
    assert log[0]["verify"] == [nv.VERIFY_SKIPPED, nv.VERIFY_SKIPPED] and log[0]["seed"] == [nv.SEED_TAKEN, nv.SEED_TAKEN]
    assert log[2]["verify"] == [nv.VERIFY_KEPT, nv.VERIFY_DROPPED | nv.VERIFY_FAIL_SUPPORT], log[2]["verify"]
    assert log[2]["seed"] == [nv.SEED_SKIPPED, nv.SEED_TAKEN] and log[2]["have"] == [1, 1]
    g1, kp = log[2]["geom"][1], det[1].double().cpu().numpy() * 2.0
    assert g1.status == 0 and g1.crop_x0 <= kp[:, 0].min() and kp[:, 0].max() < g1.crop_x1
    assert g1.crop_y0 <= kp[:, 1].min() and kp[:, 1].max() < g1.crop_y1 and g1.crop_x0 > 320 - 150 and g1.crop_y0 > 240 - 150
    g1 = log[1]["geom"][1]
    assert g1.crop_x1 <= 320 and g1.crop_y1 <= 240                                          # frame 1 (no detection) still cropped top-left
    for t in range(4):                                                                       # stream 0 is untouched by the verification
        assert torch.equal(bits(log[t]["kp2d"][0]), bits(plog[t]["kp2d"][0])), t
        a, b = log[t]["geom"][0], plog[t]["geom"][0]
        assert bytes(a) == bytes(b), t
    assert trk.verify_counts.cpu()[:, 3].tolist() == [int(O.ellipse(240, 320, 240.0, 180.0, 60.0, 50.0).sum())] * 2
    # an empty mask: nothing to compare, nothing changes
    before = (trk.kp2d.clone(), trk.have.clone())
    empty[0] = True
    assert trk.acquire(frames[3]).cpu().tolist() == [nv.SEED_SKIPPED, nv.SEED_SKIPPED]
    assert trk.verify_status.cpu().tolist() == [nv.VERIFY_UNDECIDED, nv.VERIFY_UNDECIDED]
    assert torch.equal(bits(trk.kp2d), bits(before[0])) and torch.equal(trk.have, before[1])
    # forced: every stream is reseeded anyway, verify is not launched
    trk.verify_status.fill_(-1)
    assert trk.acquire(frames[3], force=True, min_prob=0.0).cpu().tolist() == [nv.SEED_TAKEN, nv.SEED_TAKEN]
    assert trk.verify_status.cpu().tolist() == [-1, -1]
    # a detector without a mask cannot be verified against
    trk.detector = lambda img: (det, None, None)
    with pytest.raises(nv.HrpError, match="mask"):
        trk.acquire(frames[3])


def test_launch_sequence_with_verification():
    xyz = xyz_of(np.array([[[300.0 + 10 * i, 200.0 + 8 * i] for i in range(7)]])).to(DEV)
    frames = torch.randint(0, 256, (1, 480, 640, 3), dtype=torch.uint8, device=DEV)
    det, mask = torch.full((1, 7, 2), 100.0, device=DEV), torch.ones(1, 1, 240, 320, device=DEV)
    names = []

    def hook(name, args, launch):
        names.append(name)
        launch()
    model = lambda reg, root, k, Kc: stub_outputs(xyz)   # noqa: E731
    on = PoseTracker(model, ROBOT, K, (480, 640), device=DEV, detector=lambda img: (det, mask, None), acquire_every=3, min_coverage=0.25)
    off = PoseTracker(model, ROBOT, K, (480, 640), device=DEV, detector=lambda img: (det, mask, None), acquire_every=3)
    step = ["hrp_track_prepare", "hrp_track_update"]
    nv.set_profile_hook(hook)
    try:
        for _ in range(4):
            on.step(frames)
        assert names == ["hrp_track_verify", "hrp_track_seed"] + step * 3 + ["hrp_track_verify", "hrp_track_seed"] + step
        del names[:]
        for _ in range(4):
            off.step(frames)
        assert names == ["hrp_track_seed"] + step * 3 + ["hrp_track_seed"] + step
    finally:
        nv.set_profile_hook(None)
    torch.cuda.synchronize()


def test_graph_replay_of_verify_and_seed_equals_eager():
    rng = np.random.default_rng(8)
    blobs = [O.ellipse(240, 320, cx, cy, 50.0, 40.0) for cx, cy in ((100.0, 80.0), (230.0, 170.0), (100.0, 80.0))]
    sets = []
    for i in range(3):
        det = torch.from_numpy((rng.uniform(40, 280, (3, 7, 2)) * [1.0, 0.75]).astype(np.float32)).to(DEV)
        m = np.stack([blobs[(i + b) % 3] for b in range(3)]).astype(np.float32) * rng.uniform(0.6, 1.0, (3, 240, 320)).astype(np.float32)
        sets.append((det, torch.from_numpy(m[:, None]).to(DEV)))
    start = np.stack([np.array([200.0, 160.0]) + rng.uniform(-1, 1, (7, 2)) * [60, 50] for _ in range(3)])     # on the first blob

    def new():
        trk = PoseTracker(None, ROBOT, K, (480, 640), streams=3, device=DEV, detector=lambda img: None, min_support=0.5, min_coverage=0.3)
        trk.reset(start[:2], streams=[0, 1])
        return trk

    def body(trk, det, mask, **kw):
        trk.verify(mask)
        trk.seed(det, mask, **kw)
    outs = lambda trk: [bits(t).clone() for t in (trk.verify_status, trk.verify_counts, trk.verify_sums, trk.seed_status, trk.kp2d, trk.have)]   # noqa: E731
    trk, eager = new(), []
    for det, mask in sets:
        body(trk, det, mask)
        eager.append(outs(trk))
    assert len({tuple(e[0].cpu().tolist()) for e in eager}) > 1 and len({tuple(e[3].cpu().tolist()) for e in eager}) > 1
    trk = new()
    bufs = [torch.zeros_like(t) for t in sets[0]]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body(trk, *bufs, min_inside=8)                  # warm-up on the capture stream: an empty mask and a refused seed change no state
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert trk.have.cpu().tolist() == [1, 1, 0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body(trk, *bufs)
    for (det, mask), want in zip(sets, eager):
        bufs[0].copy_(det)
        bufs[1].copy_(mask)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs(trk), want))


# ---- the silhouette ------------------------------------------------------------------------------------------------------------
SH, SW = 60, 80                                      # the detector's (and the renderer's) maps; frames are 120 x 160
KS = np.array([[140.0, 0, 80.0], [0, 140.0, 60.0], [0, 0, 1.0]])


def box_mesh(seed=3, n=3):
    """One box per visual-mesh link, every side an n x n grid of quads: 9 * 6 * 2 n^2 = 972 triangles at n = 3."""
    g = np.random.Generator(np.random.PCG64(seed))
    lin = np.linspace(-1.0, 1.0, n + 1, dtype=np.float32)
    verts, links, faces = [], [], []
    for link in range(9):
        half, off = g.uniform(0.03, 0.08, 3).astype(np.float32), g.uniform(-0.03, 0.03, 3).astype(np.float32)
        for axis in range(3):
            for sign in (-1.0, 1.0):
                base = sum(len(v) for v in verts)
                a, b = np.meshgrid(lin, lin, indexing="ij")
                p = np.zeros(((n + 1) ** 2, 3), np.float32)
                p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = sign, a.reshape(-1), b.reshape(-1)
                verts.append(p * half + off)
                links += [link] * len(p)
                for i in range(n):
                    for j in range(n):
                        v00 = base + i * (n + 1) + j
                        faces += [(v00, v00 + 1, v00 + n + 2), (v00, v00 + n + 2, v00 + n + 1)]
    return torch.tensor(np.concatenate(verts)), torch.tensor(np.asarray(links, np.uint8)), torch.tensor(np.asarray(faces, np.int32))


class _Scene:
    """A tracker with a box-mesh renderer whose model stub predicts the poses of tests/golden/golden_mesh_pose.npz."""

    def __init__(self, **kw):
        from hrpe_amd.lib.utils.urdf_robot import URDFRobot
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_mesh_pose.npz"))
        q, r6, t = [torch.tensor(g[k]).float()[:2] for k in ("q", "rot6d", "t")]
        t = t.clone()
        t[:, 2] = t[:, 2].abs()
        self.q, self.r6, self.t = q.to(DEV), r6.to(DEV), t.to(DEV)
        self.B = B = q.shape[0]
        self.robot = URDFRobot("panda")
        self.renderer = self.robot.set_robot_renderer(torch.tensor(KS), (2 * SH, 2 * SW), scale=0.5, device=DEV,
                                                      mesh=tuple(m.to(DEV) for m in box_mesh()))
        self.xyz = self.robot.get_keypoints_root(self.q, self.r6, self.t, root=3).detach()
        nkp = self.xyz.shape[1]
        z = lambda *s: torch.zeros(B, *s, device=DEV)   # noqa: E731
        self.model = lambda reg, root, k, Kc: (self.q, self.r6, self.t, z(2), z(1), z(nkp, 3), z(nkp, 3), self.xyz)
        self.det = torch.tensor([[[20.0 + 5 * i, 15.0 + 4 * i] for i in range(nkp)]] * B, device=DEV)
        self.mask = torch.zeros(B, 1, SH, SW, device=DEV)
        self.frames = torch.randint(0, 256, (B, 2 * SH, 2 * SW, 3), dtype=torch.uint8, device=DEV)
        self.trk = PoseTracker(self.model, self.robot, KS, (2 * SH, 2 * SW), streams=B, rootnet_resize_hw=(64, 64), other_resize_hw=(64, 64),
                               device=DEV, detector=lambda img: (self.det, self.mask, None), detector_scale=0.5, min_iou=0.5,
                               renderer=self.renderer, reference_keypoint_id=3, **kw)

    def alpha(self):
        with torch.no_grad():
            return self.robot.get_rendered_masks(self.q, self.r6, self.t, self.renderer, root=3)


def _no_sync_step(trk, frames):
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            trk.step(frames)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert not [str(w.message) for w in rec if "synchron" in str(w.message).lower()], [str(w.message) for w in rec]


def test_step_with_verification_does_not_synchronise():
    xyz, det, mask = _loop_pieces()
    frames = torch.randint(0, 256, (2, 480, 640, 3), dtype=torch.uint8, device=DEV)
    trk = PoseTracker(lambda reg, root, k, Kc: stub_outputs(xyz), ROBOT, K, (480, 640), streams=2, rootnet_resize_hw=(64, 64),
                      other_resize_hw=(64, 64), device=DEV, detector=lambda img: (det, mask, None), acquire_every=1, min_support=0.5,
                      min_coverage=0.1)
    for _ in range(2):
        trk.step(frames)
    _no_sync_step(trk, frames)
    assert trk.verify_status.cpu().tolist() == [nv.VERIFY_KEPT, nv.VERIFY_DROPPED | nv.VERIFY_FAIL_SUPPORT | nv.VERIFY_FAIL_COVERAGE]
    sc = _Scene(acquire_every=1)                         # the rendered silhouette in the step
    sc.mask.copy_((sc.alpha() > 0.5).float()[:, None])
    names = []

    def hook(name, args, launch):
        names.append(name)
        launch()
    for _ in range(2):                                   # (the first render checks the mesh's index ranges once, with a read-back)
        sc.trk.step(sc.frames)
    nv.set_profile_hook(hook)
    try:
        _no_sync_step(sc.trk, sc.frames)
    finally:
        nv.set_profile_hook(None)
    assert names == ["hrp_mesh_pose", "hrp_silhouette_fwd", "hrp_track_verify", "hrp_track_seed", "hrp_track_prepare", "hrp_track_update"], names


def test_silhouette_iou():
    sc = _Scene()
    trk, B, n = sc.trk, sc.B, SH * SW
    alpha = sc.alpha()
    assert tuple(alpha.shape) == (B, SH, SW) and torch.equal(alpha, sc.alpha())              # deterministic: the same tensor again
    binary = (alpha > 0.5).float()
    assert all(int(v) >= 64 for v in binary.sum((1, 2)).tolist())                             # the robot is in every picture
    trk.step(sc.frames)                                                                       # the state is now the prediction

    def expect(mask):
        m, a = mask.double(), alpha.double()
        want = torch.stack([(m * a).sum((1, 2)), m.sum((1, 2)), a.sum((1, 2))], 1).cpu().numpy()
        got = trk.verify_sums.cpu().numpy()
        for b in range(B):
            assert O.sums_ok(got[b], want[b], n, False), (b, got[b], want[b])
        return want[:, 0] / (want[:, 1] + want[:, 2] - want[:, 0])
    sc.mask.copy_(binary[:, None])
    trk.acquire(sc.frames)
    iou = expect(binary)
    assert (iou > 0.9).all() and trk.verify_status.cpu().tolist() == [nv.VERIFY_KEPT] * B, (iou, trk.verify_status)
    assert trk.seed_status.cpu().tolist() == [nv.SEED_SKIPPED] * B
    trk.step(sc.frames)
    shifted = torch.roll(binary, (SH // 2, SW // 2), (1, 2))
    sc.mask.copy_(shifted[:, None])
    trk.acquire(sc.frames)
    iou = expect(shifted)
    assert (iou < 0.4).all() and trk.verify_status.cpu().tolist() == [nv.VERIFY_DROPPED | nv.VERIFY_FAIL_IOU] * B, (iou, trk.verify_status)
    assert trk.have.cpu().tolist() == [int(v == nv.SEED_TAKEN) for v in trk.seed_status.cpu().tolist()]      # dropped, then seed's own checks
    # after reset(kp2d) the state is not the last prediction: no silhouette, the IoU criterion is off for that call
    trk.step(sc.frames)
    trk.reset(trk.kp2d.clone())
    names = []

    def hook(name, args, launch):
        names.append(name)
        launch()
    nv.set_profile_hook(hook)
    try:
        trk.acquire(sc.frames)
    finally:
        nv.set_profile_hook(None)
    assert names == ["hrp_track_verify", "hrp_track_seed"], names
    assert trk.verify_status.cpu().tolist() == [nv.VERIFY_KEPT] * B and trk.verify_sums.cpu()[:, [0, 2]].abs().max().item() == 0.0
    # the renderer's size is checked against the mask's on the host
    trk.step(sc.frames)
    trk.detector = lambda img: (sc.det, sc.mask[..., :SW - 1], None)
    with pytest.raises(nv.HrpError, match="renderer"):
        trk.acquire(sc.frames)
