"""Generate tests/golden/golden_kp_readout.npz: the reference's own key-point read-out on the exact operands of
tests/kp_readout_oracle.py, in fp32 on the CPU as it ships.

Run by hand where the reference tree exists:  ``python tests/golden/gen_golden_kp_readout.py``

The two reference classes, ``KeypointUpSample`` and ``SpatialSoftArgmax`` (lib/models/ctrnet/keypoint_seg_resnet.py:10-100), are
imported from the reference file itself (torchvision stubbed by ref_harness: the file imports torchvision.models at the top and these
two classes use none of it) and lines 137-143 of ``KeyPointSegNet.forward`` are replayed on them: read_out, spatialsoftargmax,
``- offset``, ``* scale``.  The operands are NOT stored: tests regenerate them from the shape (kp_readout_oracle.operands seeds its
generator from the shape), as golden_integral.npz does.  Stored per case <key>: <key>_kp [B, k, 2] f32 (the reference's output),
<key>_heat_max [B, k] f32, <key>_shape, <key>_s, <key>_seed; once: lim, size.  The generator also asserts what the tests rely on:
the reference's fp32 heat-map equals the float64 one bit for bit on these operands, and prints the reference's own key-point error
against float64 in normalised units."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402
import kp_readout_oracle as O  # noqa: E402

STRIP = 1        # HRP_KP_STRIP_ROWS when the fixture was written (the seam shapes follow it; tests fall back to the oracle otherwise)


def reference_classes():
    rh._install_stubs()
    path = os.path.join(rh.REFERENCE_ROOT, "lib", "models", "ctrnet", "keypoint_seg_resnet.py")
    spec = importlib.util.spec_from_file_location("ref_keypoint_seg_resnet", path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod.KeypointUpSample, mod.SpatialSoftArgmax


def main():
    KeypointUpSample, SpatialSoftArgmax = reference_classes()
    out = dict(lim=np.array(O.LIM, np.float32), size=np.array(O.SIZE, np.int64), strip=np.int64(STRIP))
    worst = 0.0
    for shape, spikes in O.all_cases(STRIP):
        x, w, b, s = O.operands(shape, spikes)
        read_out = KeypointUpSample(shape[1], shape[2])
        with torch.no_grad():
            read_out.kps_score_lowres.weight.copy_(w.float())
            read_out.kps_score_lowres.bias.copy_(b.float())
            heat = read_out(x.float())                                       # line 137
            keypoints = SpatialSoftArgmax()(heat)                            # line 138
            offset = torch.tensor([O.LIM[0], O.LIM[2]])                      # line 140
            scale = torch.tensor([O.SIZE[0] // 2, O.SIZE[1] // 2])           # line 141
            norm = keypoints.clone()
            keypoints = keypoints - offset                                   # line 142
            keypoints = keypoints * scale                                    # line 143
        want = O.readout64(x, w, b)
        assert torch.equal(heat.double(), want["heat"]), (shape, "the reference's fp32 heat-map is not exact on these operands")
        n64 = want["kp"] / torch.tensor([O.SIZE[0] // 2, O.SIZE[1] // 2]).double() + torch.tensor([O.LIM[0], O.LIM[2]]).double()
        err = float((norm.double() - n64).abs().max())
        worst = max(worst, err)
        print(f"{O.key(shape, spikes):24s} s {s}  pmax {float(want['pmax'].max()):.3f}  reference - float64 (normalised) {err:.2e}")
        k = O.key(shape, spikes)
        out[k + "_kp"] = keypoints.numpy().astype(np.float32)
        out[k + "_heat_max"] = heat.amax(dim=(2, 3)).numpy().astype(np.float32)
        out[k + "_shape"] = np.array(shape, np.int64)
        out[k + "_s"] = np.int64(s)
        out[k + "_seed"] = np.int64(O.seed_of(shape, spikes))
    print(f"worst reference error {worst:.2e} normalised units")
    dst = os.path.join(HERE, "golden_kp_readout.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
