"""Generate tests/golden/golden_lr_schedule.npz: the learning rates that the reference's own ``get_scheduler``
(lib/utils/utils.py:147-189) gives a ``torch.optim.Adam`` on a CPU parameter.

Run by hand where the reference tree exists:  ``python tests/golden/gen_golden_schedule.py``

What runs is the reference's function.  Shells, as in the other generators: the imports at the top of its utils.py that are absent
here or drag the dataset stack in (``lib.dataset.*`` loaders, tensorboard, torchnet, tqdm) are empty modules with the imported names;
``get_scheduler`` touches none of them.

Per schedule ``<name>`` (the config numbers are stored beside the rates, as ``<name>:cfg:<key>``):
  ``<name>:lr0``          the rate right after the scheduler is built on a fresh optimizer (lr = 1e-4, last_epoch = -1)
  ``<name>:lr``           the rate after each of ``steps`` calls of ``lr_scheduler.step()`` (``end_decay + 5`` unless truncated)
  ``<name>:resumed:lr0``  the rate right after ``get_scheduler(args, optimizer, 50)`` on an optimizer that loaded the state dict
                          (with its ``initial_lr``) saved after 50 scheduler steps of the run above
  ``<name>:resumed:lr``   and after each further call, up to ``max(steps, 55)`` epochs in all
``unknown_schedule_type``: the name of the exception the reference raises for ``use_schedule`` with a type that is none of the three.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.setup()
import torch  # noqa: E402

LR, RESUME = 1e-4, 50

SCHEDULES = {
    "exponential_panda": dict(cfg=dict(schedule_type="exponential", n_epochs_warmup=0, start_decay=45, end_decay=100, exponent=0.95), steps=105),
    "exponential_orb": dict(cfg=dict(schedule_type="exponential", n_epochs_warmup=0, start_decay=20, end_decay=300, exponent=0.78), steps=60),
    "linear_depthnet": dict(cfg=dict(schedule_type="linear", n_epochs_warmup=15, start_decay=100, end_decay=300, final_decay=0.01), steps=305),
    "everyXepoch": dict(cfg=dict(schedule_type="everyXepoch", step=10, step_decay=0.5, end_decay=35), steps=40),
}


def import_reference_get_scheduler():
    shells = {"lib.dataset.multiepoch_dataloader": ["MultiEpochDataLoader"], "lib.dataset.samplers": ["PartialSampler"],
              "lib.dataset.dream": ["DreamDataset"], "torch.utils.tensorboard": ["SummaryWriter"], "torchnet": [],
              "torchnet.meter": ["AverageValueMeter"], "tqdm": ["tqdm"]}
    for name, attrs in shells.items():
        if not name.startswith("lib."):
            try:
                __import__(name)
                continue
            except ImportError:
                pass
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, None)
        sys.modules[name] = m
    from lib.utils.utils import get_scheduler
    return get_scheduler


def rates(opt):
    return [g["lr"] for g in opt.param_groups]


def main():
    get_scheduler = import_reference_get_scheduler()
    out = {"lr": np.float64(LR), "resume_epoch": np.int64(RESUME)}
    for name, spec in SCHEDULES.items():
        args = rh._AttrDict(use_schedule=True, **spec["cfg"])
        steps = spec["steps"]
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=LR)
        sched = get_scheduler(args, opt, -1)
        out[f"{name}:lr0"] = np.float64(rates(opt)[0])
        seq, saved = [], None
        total = max(steps, RESUME + 5)             # (a schedule that ends before the resume epoch is run on to it, and 5 past it)
        for e in range(total):
            opt.step()
            sched.step()
            seq.append(rates(opt)[0])
            if e + 1 == RESUME:
                saved = opt.state_dict()
        out[f"{name}:lr"] = np.array(seq[:steps], np.float64)
        assert "initial_lr" in saved["param_groups"][0]
        opt2 = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1.0)     # the rate comes from the state dict
        opt2.load_state_dict(saved)
        sched2 = get_scheduler(args, opt2, RESUME)
        out[f"{name}:resumed:lr0"] = np.float64(rates(opt2)[0])
        seq2 = []
        for e in range(RESUME, total):
            opt2.step()
            sched2.step()
            seq2.append(rates(opt2)[0])
        out[f"{name}:resumed:lr"] = np.array(seq2, np.float64)
        for k, v in spec["cfg"].items():
            out[f"{name}:cfg:{k}"] = np.array(v)
        out[f"{name}:cfg:steps"] = np.int64(steps)
        print(f"{name}: lr0 {out[f'{name}:lr0']:.3e}, last {seq[-1]:.6e}, resumed lr0 {out[f'{name}:resumed:lr0']:.6e}, "
              f"resumed last {seq2[-1] if seq2 else float('nan'):.6e}")
    assert get_scheduler(rh._AttrDict(use_schedule=False), None, -1) is None
    try:                                            # a schedule_type that is none of the three: record what the reference does
        get_scheduler(rh._AttrDict(use_schedule=True, schedule_type="cosine"), opt, -1)
        out["unknown_schedule_type"] = np.array("returns")
    except Exception as e:                          # noqa: BLE001
        out["unknown_schedule_type"] = np.array(type(e).__name__)
    print("unknown schedule_type:", out["unknown_schedule_type"])
    path = os.path.join(HERE, "golden_lr_schedule.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
