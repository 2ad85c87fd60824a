"""Optimizer step of the reference's training loops on the HIP path.

The reference trains with ``torch.optim.Adam`` preceded by ``torch.nn.utils.clip_grad_norm_``
(scripts/train_full.py:42, configs/panda/full.yaml:39 ``clip_gradient: 5``).  ``FusedClipAdam`` is that pair
as two table-driven launches over ALL parameters (hrp_opt_grad_sumsq, hrp_opt_adam_step in include/hrp.h):
the multi-tensor torch path spends ~70 launches and 3 ms per step on the 57 M parameters of the full
network, this one ~0.6 ms.  Same arithmetic as torch (fp32 state, bias correction from a device-side step
counter so that the step is capturable into a HIP graph), no amsgrad (the reference does not use it).  There is no
CPU path.

It is a ``torch.optim.Optimizer``: ``param_groups`` / ``state_dict()`` / ``load_state_dict()`` use torch.optim.Adam's
layout (per-parameter ``step``, ``exp_avg``, ``exp_avg_sq``), so the ``optimizer_state_dict`` of the reference's
checkpoints (lib/utils/utils.py:192-267 ``resume_run`` / ``save_checkpoint``) loads into it and what it saves loads
into ``torch.optim.Adam``.

Two paths.  Called with one list of parameters, floats and no weight decay, the step is ``hrp_opt_adam_step``: the
hyper-parameters are launch arguments, read from ``param_groups[0]`` at every eager step and BAKED into a captured HIP
graph.  A list of group dicts, a non-zero ``weight_decay`` or ``device_hyper=True`` selects ``hrp_opt_adam_step_groups``:
the groups' ``lr / betas / eps / weight_decay`` live in a device table that the kernel reads when it runs, and
``publish_hyper()`` writes the rows that changed (``hrp_opt_set_group``, on the current stream).  ``LambdaLR``
(utils.py:147-189, ``hrpe_amd.lib.utils.utils.get_scheduler``) can drive ``param_groups[i]["lr"]`` on both paths in an eager
loop; through a replayed graph only the second path applies the scheduled rate:
``graph.replay(); lr_scheduler.step(); optimizer.publish_hyper()`` (get_scheduler's scheduler does the last call itself).
"""
import ctypes as C

import torch

from . import _native as nv


class FusedClipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None, weight_decay=0.0, device_hyper=False):
        params = list(params)
        grouped = any(isinstance(p, dict) for p in params)
        if grouped:
            if not all(isinstance(p, dict) for p in params):
                raise ValueError("FusedClipAdam: either parameters or parameter-group dicts, not both")
            params = [dict(g, params=[p for p in g["params"] if p.requires_grad]) for g in params]
            params = [g for g in params if g["params"]]
        else:
            params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("FusedClipAdam: no parameters")
        # the device-table path (module docstring); without it nothing differs from the one-group class: same defaults, same launches
        self._device_hyper = bool(grouped or device_hyper or weight_decay)
        super().__init__(params, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                                      weight_decay=float(weight_decay) if self._device_hyper else 0, amsgrad=False,
                                      maximize=False, foreach=None, capturable=True, differentiable=False, fused=None))
        for g in self.param_groups:
            if g["amsgrad"] or g["maximize"]:
                raise ValueError("FusedClipAdam: amsgrad / maximize are not supported")
        self.params = [p for g in self.param_groups for p in g["params"]] if self._device_hyper else self.param_groups[0]["params"]
        dev = self.params[0].device
        if dev.type != "cuda":
            raise nv.HrpError("FusedClipAdam runs on an MI355X (gfx950) only; there is no CPU path")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("FusedClipAdam: parameters must be contiguous fp32 tensors on one device")
        self.device = dev
        self.max_norm = float(max_norm) if max_norm else 0.0
        total = sum((p.numel() + 3) // 4 * 4 for p in self.params)
        self._m = torch.zeros(total, dtype=torch.float32, device=dev)
        self._v = torch.zeros(total, dtype=torch.float32, device=dev)
        self.state_views, off = [], 0
        for p in self.params:
            n = p.numel()
            self.state_views.append((self._m[off:off + n].view_as(p), self._v[off:off + n].view_as(p)))
            off += (n + 3) // 4 * 4
        self.step_count = torch.zeros(1, dtype=torch.float32, device=dev)
        self._publish_state()
        self._slots = torch.zeros(8, dtype=torch.float32, device=dev)
        self._chunk_sums = None
        self._grad_ptrs = None
        self._tensors = self._chunks = None
        self._nchunks = 0
        if self._device_hyper:
            ng = len(self.param_groups)
            self._groups = torch.zeros(ng * C.sizeof(nv.OptGroup) // 4, dtype=torch.float32, device=dev)
            self._tensor_group = torch.tensor([i for i, g in enumerate(self.param_groups) for _ in g["params"]],
                                              dtype=torch.int32, device=dev)
            self._hyper_mirror = [None] * ng          # what the device table holds, per group
            self.publish_hyper()

    def _hyper(self, g):
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))

    def hyper_is_stale(self):
        """True when some group's lr / betas / eps / weight_decay differ from what the device table was last given."""
        return self._device_hyper and any(self._hyper(g) != m for g, m in zip(self.param_groups, self._hyper_mirror))

    def publish_hyper(self):
        """Write the groups whose ``param_groups`` values changed into the device table (one tiny launch each, on the
        current stream, so it is ordered after a replay issued there).  Nothing to do on the launch-argument path.  Not
        during a capture: a captured setter would rewrite the captured values at every replay."""
        if not self._device_hyper:
            return
        s = None
        for i, g in enumerate(self.param_groups):
            h = self._hyper(g)
            if h == self._hyper_mirror[i]:
                continue
            if s is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("FusedClipAdam.publish_hyper() during a HIP graph capture: publish before the capture "
                                       "and after every replay")
                s = torch.cuda.current_stream(self.device).cuda_stream
            nv.call("hrp_opt_set_group", self._groups.data_ptr(), len(self.param_groups), i, *h, s)
            self._hyper_mirror[i] = h

    def _publish_state(self):
        """torch.optim.Adam's per-parameter state, as views of the flat moment buffers and the shared step counter."""
        for p, (m, v) in zip(self.params, self.state_views):
            self.state[p] = {"step": self.step_count.view(()), "exp_avg": m, "exp_avg_sq": v}

    def state_dict(self):
        """torch.optim.Adam's layout; every parameter gets its OWN step tensor (the foreach Adam increments them
        one by one, aliases of the shared counter would advance N steps at a time)."""
        sd = super().state_dict()
        sd["state"] = {k: dict(v, step=v["step"].clone()) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Accepts torch.optim.Adam's (or this class's) state_dict: moments are copied into the flat buffers."""
        if not self._device_hyper and len(state_dict["param_groups"]) != 1:
            raise ValueError("FusedClipAdam: one parameter group only")
        for g in state_dict["param_groups"]:
            if self._device_hyper:
                if g.get("amsgrad", False) or g.get("maximize", False):
                    raise ValueError("FusedClipAdam: amsgrad / maximize are not supported")
            elif g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("FusedClipAdam: weight_decay / amsgrad / maximize are not supported")
        super().load_state_dict(state_dict)
        steps = set()
        with torch.no_grad():
            for p, (m, v) in zip(self.params, self.state_views):
                st = self.state.get(p)
                if not st:               # torch leaves parameters that never stepped without state
                    m.zero_()
                    v.zero_()
                    continue
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
                steps.add(float(st["step"]))
            if len(steps) > 1:
                raise ValueError(f"FusedClipAdam: parameters at different step counts {sorted(steps)}")
            self.step_count.fill_(steps.pop() if steps else 0.0)
        for g in self.param_groups:
            g["capturable"] = True
        self._publish_state()

    def _build_tables(self):
        ptrs = tuple(p.grad.data_ptr() for p in self.params)
        if ptrs == self._grad_ptrs:
            return
        tab = (nv.OptTensor * len(self.params))()
        chunks = []
        for i, (p, (m, v)) in enumerate(zip(self.params, self.state_views)):
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous():
                raise ValueError("FusedClipAdam: gradients must be contiguous fp32")
            tab[i].param, tab[i].grad, tab[i].exp_avg, tab[i].exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            tab[i].numel = p.numel()
            chunks += [(i, k) for k in range((p.numel() + nv.OPT_CHUNK - 1) // nv.OPT_CHUNK)]
        ck = (nv.OptChunk * len(chunks))()
        for j, (i, k) in enumerate(chunks):
            ck[j].tensor, ck[j].offset = i, k
        self._tensors = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.device)
        self._chunks = torch.frombuffer(bytearray(bytes(ck)), dtype=torch.uint8).to(self.device)
        self._nchunks = len(chunks)
        self._chunk_sums = torch.zeros(self._nchunks, dtype=torch.float32, device=self.device)
        self._grad_ptrs = ptrs

    def prepare(self):
        """Build the device tables (call once outside a HIP graph capture; gradients must exist)."""
        if any(p.grad is None for p in self.params):
            raise ValueError("FusedClipAdam: every parameter needs a gradient (run one backward first)")
        self._build_tables()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedClipAdam: closures are not supported")
        if self._device_hyper:
            if not torch.cuda.is_current_stream_capturing():
                self.publish_hyper()
            elif self.hyper_is_stale():
                raise RuntimeError("FusedClipAdam: param_groups changed since the device table was written and a HIP graph is being "
                                   "captured; call publish_hyper() before the capture (and after every replay)")
        self.prepare()
        g = self.param_groups[0]
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.step_count += 1
        if self.max_norm > 0:
            # per-chunk sums folded in a fixed order (no atomics): every data-parallel rank derives the same clip
            # coefficient, bit for bit, from the same averaged gradients - replicas stay identical
            nv.call("hrp_opt_grad_sumsq", self._tensors.data_ptr(), self._chunks.data_ptr(), self._nchunks,
                    self._slots.data_ptr(), self._chunk_sums.data_ptr(), s)
        if self._device_hyper:
            nv.call("hrp_opt_adam_step_groups", self._tensors.data_ptr(), self._chunks.data_ptr(), self._nchunks,
                    self._slots.data_ptr(), self.max_norm, self.step_count.data_ptr(),
                    self._groups.data_ptr(), len(self.param_groups), self._tensor_group.data_ptr(), s)
        else:
            nv.call("hrp_opt_adam_step", self._tensors.data_ptr(), self._chunks.data_ptr(), self._nchunks,
                    self._slots.data_ptr(), self.max_norm, self.step_count.data_ptr(),
                    float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), s)
        # the parameters changed through raw pointers (no tensor._version bump): inference plans must repack / refold
        from .plan import bump_param_epoch
        bump_param_epoch()

    def total_norm(self):
        """Gradient norm of the last step (before clipping), as clip_grad_norm_ returns it."""
        return self._slots.sum().sqrt()

    def zero_grad(self, set_to_none=False):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()
