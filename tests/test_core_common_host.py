"""Host-side checks of what the three trainers share (hrpe_amd.lib.core.common); no GPU needed.  Everything here is compared
bit for bit: the helpers restate arithmetic the trainers' own tests pin (k_values at rtol 2^-22, meters with ==, capacities exactly)."""
import numpy as np
import pytest
import torch

from hrpe_amd.lib.core import common as cm
from hrpe_amd.lib.core.depthnet import compute_depthnet_k_values
from hrpe_amd.lib.core.function import compute_k_values


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("axis", [0, 1])
def test_grown(axis, dtype):
    t = torch.arange(1, 4 * 6 + 1).reshape(4, 6).to(dtype)
    old, used = t.shape[axis], 3
    # room enough: the same object, whatever ``used`` says
    assert cm.grown(t, axis, used, old) is t and cm.grown(t, axis, used, 1) is t
    for need in (old + 1, 2 * old, 2 * old + 5):
        g = cm.grown(t, axis, used, need)
        assert g is not t and g.dtype == t.dtype and g.device == t.device
        want = list(t.shape)
        want[axis] = max(need, 2 * old)
        assert list(g.shape) == want
        assert torch.equal(g.narrow(axis, 0, used), t.narrow(axis, 0, used))
        assert (g.narrow(axis, used, want[axis] - used) == 0).all()         # past ``used``: zeros, not the old entries
    assert torch.equal(t, torch.arange(1, 25).reshape(4, 6).to(dtype))      # the source is left as it was


def test_compute_k_values_is_the_two_formulas_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    fx = torch.tensor([615.25, -320.5, 1066.778, -0.37, 555.5])             # negative fx: a mirrored camera, as in the fixtures
    fy = torch.tensor([614.75, 320.5, -1067.487, -0.91, 555.5])
    x1, y1 = torch.rand(5, generator=g) * 300, torch.rand(5, generator=g) * 200
    bboxes = torch.stack([x1, y1, x1 + torch.rand(5, generator=g) * 317 + 1, y1 + torch.rand(5, generator=g) * 259 + 1], dim=1)
    bboxes[2] = bboxes[2, [2, 3, 0, 1]]                                     # corners the other way round
    for real_bbox in ((1000.0, 1000.0), (1300.0, 700.0)):
        area = torch.max(torch.abs(bboxes[:, 2] - bboxes[:, 0]), torch.abs(bboxes[:, 3] - bboxes[:, 1])) ** 2
        plain = torch.sqrt(fx * fy * real_bbox[0] * real_bbox[1] / area).to(torch.float32)
        absolute = torch.sqrt(torch.abs(fx) * torch.abs(fy) * real_bbox[0] * real_bbox[1] / area).to(torch.float32)
        for got in (cm.compute_k_values(fx, fy, bboxes, real_bbox), compute_k_values(fx, fy, bboxes, real_bbox)):
            assert torch.equal(got.nan_to_num(-1.0), plain.nan_to_num(-1.0))
        for got in (cm.compute_k_values(fx, fy, bboxes, real_bbox, absolute=True), compute_depthnet_k_values(fx, fy, bboxes, real_bbox)):
            assert torch.equal(got, absolute)
    # one negative focal length: the plain form is NaN as the reference's is, the absolute form is not
    assert torch.isnan(plain[[1, 2]]).all() and torch.isfinite(plain[[0, 3, 4]]).all() and torch.isfinite(absolute).all()


def test_meter_mean_is_the_sequential_fp64_sum():
    rows = torch.randn(3, 12, generator=torch.Generator().manual_seed(5))
    acc = np.zeros(12, np.float64)
    for r in rows.double().numpy():
        acc = acc + r
    want = acc / 3
    for given in (rows, rows.numpy(), rows.double().numpy()):
        got = cm.meter_mean(given)
        assert got.dtype == np.float64 and got.shape == (12,) and (got == want).all()
    # the fp32 mean of the same rows is another number in the last bit, in every column of this seed
    assert (np.mean(rows.numpy(), axis=0).astype(np.float64) != want).all()
    # one value per batch (DepthEvaluator's losses): a scalar
    assert cm.meter_mean(rows[:, 0].numpy()) == want[0]


class _Dataset:
    def __init__(self):
        self.calls = []

    def to_device(self, sample, device=None):
        self.calls.append((sample["n"], device))
        return dict(sample, moved=True)


class _Loader:
    def __init__(self, samples, dataset):
        self.samples, self.dataset = samples, dataset

    def __iter__(self):
        return iter(self.samples)


class _Sized(_Dataset):
    def __len__(self):
        return 37


def test_validation_batches_and_loader_capacity():
    samples = [dict(n=0, frame=1, aug=2), dict(n=1, frame=1), dict(n=2, root={}), dict(n=3, aug=2, frame=0)]
    # a list has no .dataset: the default capacity, samples in the reference schema pass as they are
    assert cm.loader_capacity(samples[1:3]) == 1024 and cm.loader_capacity([], default=5) == 5
    out = list(cm.validation_batches(samples[1:3], "cpu"))
    assert len(out) == 2 and out[0] is samples[1] and out[1] is samples[2]
    # a dataset without __len__: the default; to_device exactly for the samples with both ``frame`` and ``aug``, in order
    ds = _Dataset()
    loader = _Loader(samples, ds)
    assert cm.loader_capacity(loader) == 1024 and cm.loader_capacity(loader, default=7) == 7
    out = list(cm.validation_batches(loader, "dev"))
    assert ds.calls == [(0, "dev"), (3, "dev")]
    assert [o["n"] for o in out] == [0, 1, 2, 3] and [o.get("moved", False) for o in out] == [True, False, False, True]
    assert out[1] is samples[1] and out[2] is samples[2]
    # a sized dataset: its length; an empty one: the default
    assert cm.loader_capacity(_Loader(samples, _Sized())) == 37
    assert cm.loader_capacity(_Loader([], [])) == 1024
