"""DreamDataset.to_device (csrc/dream.hip) on the GPU against the reference's recorded images (tests/golden/golden_dream.npz):
every byte of every case, batched, reproducible, under graph replay, through prepare_batch and one eval forward."""
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
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.dataset import dream as D  # noqa: E402
from test_dream_host import CASES, GOLD, need_frame, run_case, scene  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def want_images(name, view):
    k = name + "/" + view + "/images"
    return GOLD[k] if k in GOLD.files else GOLD[name + "/root/images"]


def device_batch(ds, items):
    batch = torch.utils.data.default_collate(items)
    out = ds.to_device(batch, DEV)
    torch.cuda.synchronize()
    return batch, out


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_bytes_equal_reference(scene, name):  # noqa: F811
    case = CASES[name]
    need_frame(scene, case)
    ds, item, _ = run_case(scene, case)
    _, out = device_batch(ds, [item])
    for v in ("root", "other"):
        got, want = out[v]["images"][0].cpu().numpy(), want_images(name, v)
        assert got.shape == want.shape and out[v]["images"].dtype == torch.uint8
        n = int((got != want).sum())
        assert n == 0, f"{name}/{v}: {n} of {got.size} bytes differ, max {np.abs(got.astype(int) - want).max()}"
    if ds.rootnet_resize_hw == ds.other_resize_hw:
        assert out["root"]["images"] is out["other"]["images"]
    assert torch.equal(out["images_original"][0].cpu(), item["frame"].permute(2, 0, 1))


def test_batched_cases_bytes_equal_reference(scene):  # noqa: F811
    """All 640 x 480, 128 x 128 cases in one batch (truncated and plain working frames of different sizes together)."""
    names = [n for n, c in sorted(CASES.items()) if c["frame"] != 4 and c["kw"].get("rootnet_resize_hw") == [128, 128]
             and c["kw"].get("other_resize_hw") == [128, 128]]
    for n in names:
        need_frame(scene, CASES[n])
    items = []
    for n in names:
        ds, item, _ = run_case(scene, CASES[n])
        items.append(item)
    _, out = device_batch(ds, items)
    got = out["root"]["images"].cpu().numpy()
    for i, n in enumerate(names):
        assert (got[i] == want_images(n, "root")).all(), n
    assert len(names) >= 12


def _train_batch(scene, B, seed, truncation=True):  # noqa: F811
    ds = D.DreamDataset(scene, process_truncation=truncation, occlu_p=1.0)
    random.seed(seed)
    np.random.seed(seed)
    items = [ds[i % 4] for i in range(B)]
    return ds, torch.utils.data.default_collate(items)


def test_reproducible_and_graph_replay(scene):  # noqa: F811
    ds, batch = _train_batch(scene, 8, 5)
    a = ds.to_device(batch, DEV)["root"]["images"].clone()
    b = ds.to_device(batch, DEV)["root"]["images"]
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    # static buffers, two launches captured into a graph, replayed on a second batch's table
    tab, noise, sbytes = D.descriptor_table(batch["aug"], batch["noise"])
    B = len(tab)
    frames = batch["frame"].to(DEV)
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    noise_d = torch.zeros(B * 480 * 640 * 3, dtype=torch.uint8, device=DEV)   # the largest possible fill
    noise_d[:len(noise)] = torch.from_numpy(np.frombuffer(noise, np.uint8).copy()).to(DEV)
    mh, mw = 480 + 2 * D.TRUNCATION_PAD, 640 + 2 * D.TRUNCATION_PAD
    scratch = torch.empty(B * mh * mw * 3, dtype=torch.uint8, device=DEV)
    lsum = torch.empty(B, nv.DREAM_BANDS, dtype=torch.int64, device=DEV)
    out = torch.empty(B, 3, 256, 256, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        D.pixel_launches(frames, table, noise_d, scratch, lsum, out, max_hw=(mh, mw))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.pixel_launches(frames, table, noise_d, scratch, lsum, out, max_hw=(mh, mw))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    _, batch2 = _train_batch(scene, 8, 6)
    tab2, noise2, _ = D.descriptor_table(batch2["aug"], batch2["noise"])
    want2 = ds.to_device(batch2, DEV)["root"]["images"].clone()
    frames.copy_(batch2["frame"].to(DEV))
    table.copy_(torch.from_numpy(tab2.view(np.uint8).copy()).to(DEV))
    noise_d[:len(noise2)] = torch.from_numpy(np.frombuffer(noise2, np.uint8).copy()).to(DEV)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2)


def _fixture_cpu_batch(names):
    """The reference's batch (float images holding 0 .. 255) for the fixture cases, as its DataLoader would collate it."""
    def st(k):
        return torch.stack([torch.as_tensor(GOLD[n + "/" + k]) for n in names])
    jn = CASES[names[0]]["joint_names"]
    b = {k: st(k) for k in ("bbox_strict_bounded_original", "bbox_gt2d_extended_original", "TCO", "K_original",
                            "keypoints_2d_original", "valid_mask", "keypoints_3d_original")}
    b["jointpose"] = {j: torch.tensor([GOLD[n + "/jointpose"][i] for n in names]) for i, j in enumerate(jn)}
    for v in ("root", "other"):
        b[v] = {k: st(v + "/" + k) for k in ("bbox_strict_bounded", "bbox_gt2d_extended", "K", "keypoints_3d", "keypoints_2d",
                                             "valid_mask_crop")}
        b[v]["images"] = torch.stack([torch.as_tensor(want_images(n, v)).float() for n in names])
    return b


@pytest.mark.parametrize("synthetic", [True, False])
def test_prepare_batch_matches_fixture_batch(scene, synthetic):  # noqa: F811
    from hrpe_amd.lib.core.function import prepare_batch
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    names = ["force_brightness", "occlusion", "train_s1_f0", "truncation_edge"]
    for n in names:
        need_frame(scene, CASES[n])
    items = []
    for n in names:
        ds, item, _ = run_case(scene, CASES[n])
        items.append(item)
    _, dev_batch = device_batch(ds, items)
    robot = URDFRobot("panda")
    a = prepare_batch(dev_batch, robot, DEV, reference_keypoint_id=3, synthetic=synthetic)
    b = prepare_batch(_fixture_cpu_batch(names), robot, DEV, reference_keypoint_id=3, synthetic=synthetic)
    for k in ("reg_images", "root_images"):
        assert a[k].dtype == torch.uint8
        assert torch.equal(a[k].float() / 255., b[k]), k
    for k in ("root_K", "other_K", "k_values"):
        assert torch.allclose(a[k], b[k], atol=1e-5, rtol=1e-6), k
    for k, v in b["gt"].items():
        assert torch.allclose(a["gt"][k], v, atol=1e-5, rtol=1e-5), k


def _model():
    from hrpe_amd.lib.dataset.const import INITIAL_JOINT_ANGLE
    from hrpe_amd.lib.models.full_net import RootNetwithRegInt

    class A(dict):
        __getattr__ = dict.__getitem__
    args = A(backbone_name="hrnet32", rootnet_backbone_name="hrnet32", other_image_size=256.0, use_rpmg=False, n_iter=4,
             p_dropout=0.0, reg_joint_map=False, joint_conv_dim=[], rotation_dim=6, direct_reg_rot=False,
             rot_iterative_matmul=False, fix_root=True, bbox_3d_shape=[1300, 1300, 1300], reference_keypoint_id=3, add_fc=False,
             multi_kp=False, kps_need_depth=None, pretrained_rootnet=None)
    init = {"robot_type": "panda", "pose_params": INITIAL_JOINT_ANGLE, "cam_params": np.eye(4), "init_pose_from_mean": True}
    torch.manual_seed(0)
    return RootNetwithRegInt(init, args)


def test_eval_forward_on_device_batch(scene):  # noqa: F811
    case = CASES["size256"]
    need_frame(scene, case)
    from hrpe_amd.lib.core.function import prepare_batch
    from hrpe_amd.lib.utils.urdf_robot import URDFRobot
    ds, item, _ = run_case(scene, case)
    _, dev_batch = device_batch(ds, [item, item])
    pb = prepare_batch(dev_batch, URDFRobot("panda"), DEV, reference_keypoint_id=3)
    m = _model().to(DEV).eval()
    with torch.no_grad():
        out = m(pb["reg_images"], pb["root_images"], pb["k_values"], pb["root_K"])
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in out)


def test_error_paths(scene):  # noqa: F811
    ds, batch = _train_batch(scene, 2, 7, truncation=False)
    with pytest.raises(nv.HrpError):
        ds.to_device(batch, "cpu")
    tab, noise, sbytes = D.descriptor_table(batch["aug"], batch["noise"])
    frames = batch["frame"].to(DEV)
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    noise_d = torch.from_numpy(np.frombuffer(noise, np.uint8).copy()).to(DEV)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=DEV)
    lsum = torch.empty(2, nv.DREAM_BANDS, dtype=torch.int64, device=DEV)
    out = torch.empty(2, 3, 256, 256, dtype=torch.uint8, device=DEV)
    with pytest.raises(nv.HrpError):       # CPU frames: no CPU path
        D.pixel_launches(batch["frame"], table, noise_d, scratch, lsum, out)
    with pytest.raises(nv.HrpError):       # a table for another batch size
        D.pixel_launches(frames, table[:100], noise_d, scratch, lsum, out)
    with pytest.raises(nv.HrpError):       # float output
        D.pixel_launches(frames, table, noise_d, scratch, lsum, out.float())
    with pytest.raises(nv.HrpError):       # the library rejects a working-frame bound below the frame
        D.pixel_launches(frames, table, noise_d, scratch, lsum, out, max_hw=(100, 100))
    bad = frames.permute(0, 2, 1, 3)
    with pytest.raises(nv.HrpError):
        D.pixel_launches(bad, table, noise_d, scratch, lsum, out)
