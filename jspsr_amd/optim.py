"""The reference's optimizers and schedules over ONE flat parameter buffer (reference: utils/common_config.py
get_optimizer :241-291 -- torch.optim.SGD / Adam / AdamW / RMSprop, configs/*.yml:71-76: AdamW, lr 1e-3, weight_decay
1e-6 -- and get_scheduler :294-368).

`GradReducer` already aliases every `.grad` into one flat fp32 buffer (the RCCL buckets); these optimizers re-point
every `.data` into a second flat buffer laid out identically, so a whole step is a single HBM-bound kernel launch
(jspsr_adamw_step: 16 B read + 12 B written per parameter; jspsr_optim_step, K11, for the others) instead of per-tensor
launches.  `state_dict()` / `load_state_dict()` of the model keep working: parameters are ordinary views.

A stock torch optimizer cannot stand in: it does not update the flat buffer the kernels and `GradReducer` are built on,
and `GraphedStep` needs the scalars in device memory (`enable_device_hyper` / `upload_hyper`).  torch's scheduler
classes refuse anything that is not a torch.optim.Optimizer, so the schedules are restated too, as closed forms over
`param_groups`.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from . import ops
from .ddp import GradReducer

_RANGE_START = (999.0, -999.0, 0.0, 0.0)       # get_gradient_range's start values (train/train_utils.py:132-133)


class _FlatOptimizer:
    """What the flat optimizers share: the flat layout, the `lr_overrides` ranges, torch-style `param_groups`, the scalars
    in device memory for graph capture, the fused gradient range, packed-weight invalidation and both checkpoint layouts.

    A subclass names its update (KIND of jspsr_optim_step), its state buffers (STATE: attribute == torch's state name, in
    the order state1, state2 of the C entry), whether torch keeps a `step` entry per parameter, and gives the scalars.

    grad_range: None, or a 4-float device tensor {min, max, count of non-finite elements, spare}.  When set, `step()`
    first resets it to {999, -999, 0, 0} with device work (a small device-to-device copy: a captured step resets it too)
    and every range's launch folds the min / max of the gradient it has just read into it (`fused_grad_range()` makes
    one).  It is an attribute and not an argument of step() so that `GraphedStep`, which calls step() without
    arguments, captures it."""

    KIND = None
    STATE = ()
    TORCH_STEP = True
    grad_range = None

    def __init__(self, reducer: GradReducer, lr, lr_overrides=None, group_extra=None):
        self.reducer = reducer
        self.flat_p = torch.empty_like(reducer.flat)
        over = {id(p): float(v) for p, v in (lr_overrides or {}).items()}
        extra = dict(group_extra or {})         # per-group scalars a schedule may move (momentum / betas), as torch keeps them
        self.param_groups = [{"lr": float(lr), "initial_lr": float(lr), "ranges": [], **extra}]
        by_lr = {}
        off = 0
        self._slices = {}                            # id(parameter) -> (offset, numel) in the flat buffers
        self._over = over
        self._group_of = {}                          # id(parameter) -> its entry of param_groups
        for p in reversed(reducer.params):          # same order as the gradient buffer
            n = p.numel()
            self._slices[id(p)] = (off, n)
            self.flat_p[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_p[off:off + n].view_as(p)
            if id(p) in over:
                g = by_lr.get(over[id(p)])
                if g is None:
                    g = by_lr[over[id(p)]] = {"lr": over[id(p)], "initial_lr": over[id(p)], "ranges": [], **extra}
                    self.param_groups.append(g)
            else:
                g = self.param_groups[0]
            # membership is recorded HERE, by identity -- not re-derived later from the groups' mutable "lr" / "initial_lr"
            # (a scheduler step or a loaded checkpoint rewrites those: ADVICE r3)
            self._group_of[id(p)] = g
            if g["ranges"] and g["ranges"][-1][1] == off:
                g["ranges"][-1][1] = off + n
            else:
                g["ranges"].append([off, off + n])
            off += n
        self.steps = 0
        ops.invalidate_packed_weights()      # the parameters now live elsewhere

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        self.param_groups[0]["lr"] = float(v)

    # -- what a subclass provides ---------------------------------------------------------------------------------------
    def _row(self, g, step):
        """The seven scalars of group `g` at step count `step`, as Python floats: lr, a, b, eps, weight decay, c1, c2
        (include/jspsr_hip.h, jspsr_optim_step)."""
        raise NotImplementedError

    def _hyper(self, g):
        """This class's hyper-parameters of group `g` as the checkpoint layouts name them."""
        raise NotImplementedError

    def _set_hyper(self, first):
        """Take the hyper-parameters from the first group of a loaded checkpoint."""
        raise NotImplementedError

    def _torch_group(self, g):
        """The remaining keys of the matching torch.optim class's param_groups entry."""
        raise NotImplementedError

    def _ensure_state(self):
        """Allocate state buffers that exist only for some settings (a momentum buffer); never under capture."""

    def _buffers(self):
        return [getattr(self, name, None) for name in self.STATE] + [None] * (2 - len(self.STATE))

    # -- scalars in device memory (graph capture: jspsr_amd/graph.py) ----------------------------------------------------
    def enable_device_hyper(self):
        """From now on the kernels read lr / betas / eps / weight decay / bias corrections from a small device tensor per
        parameter group (jspsr_adamw_step_dev) that `upload_hyper()` refreshes -- the launches can then be captured in a
        hipGraph and replayed while the learning rate and the step count move on.  Same arithmetic, same bits -- also when
        the host runs ahead of the GPU: every step reads the row that was uploaded for it, however many steps are queued
        (see `upload_hyper`)."""
        if getattr(self, "_hyper_dev", None) is None:
            self._hyper_dev = torch.zeros((len(self.param_groups), 8), dtype=torch.float32, device=self.flat_p.device)
        return self

    def upload_hyper(self, step=None):
        """Write the seven scalars of every group for step count `step` (default: the current one) into the device tensor;
        an ordinary stream-ordered copy from pinned memory -- call it OUTSIDE a captured region.

        The copy may still be queued behind GPU work when the next call comes (a loop that synchronises once per epoch,
        `GraphedStep` replays), so the host rows it reads are never written again: every call fills a NEW pinned tensor.
        The caching host allocator records the copy's stream on that block and hands it out again only once the copy has
        run; a call neither waits for the GPU nor, in the steady state, allocates."""
        step = self.steps if step is None else step
        rows = [list(self._row(g, step)) + [0.0] for g in self.param_groups]
        host = torch.empty((len(rows), 8), dtype=torch.float32, pin_memory=True)
        host.copy_(torch.tensor(rows, dtype=torch.float64))      # rounds to fp32, as the argument form's C floats do
        self._hyper_dev.copy_(host, non_blocking=True)

    # -- the fused gradient range ------------------------------------------------------------------------------------
    def fused_grad_range(self):
        """Make (once) and return `grad_range`: from the next step on, every step leaves the range of its gradients there."""
        if self.grad_range is None:
            self.grad_range = torch.tensor(_RANGE_START, dtype=torch.float32, device=self.flat_p.device)
        return self.grad_range

    def _range_args(self, lib):
        """(pointer to grad_range or None, pointer to the partials' workspace or None), after resetting the range."""
        r = self.grad_range
        if r is None:
            return None, None
        if r.dtype != torch.float32 or r.numel() != 4 or r.device != self.flat_p.device or not r.is_contiguous():
            raise ValueError(f"{type(self).__name__}.grad_range: a contiguous 4-float tensor on {self.flat_p.device}")
        if getattr(self, "_range_ws", None) is None:
            self._range_ws = torch.empty(lib.jspsr_optim_workspace_bytes() // 4, dtype=torch.float32, device=r.device)
            self._range_start = torch.tensor(_RANGE_START, dtype=torch.float32, device=r.device)
        r.copy_(self._range_start)
        return r.data_ptr(), self._range_ws.data_ptr()

    def step(self):
        name = type(self).__name__
        if not self.flat_p.is_cuda:
            raise RuntimeError(f"{name} runs on the GPU only")
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self._ensure_state()
        self.steps += 1
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        dev = getattr(self, "_hyper_dev", None)
        if dev is not None and not capturing:
            self.upload_hyper()                 # (under capture the owner of the graph uploads before every replay)
        self._launch(lib, stream, dev)
        ops.invalidate_packed_weights()      # the kernel wrote the parameters through raw pointers ...
        if ops.repack_after_step:
            ops.repack_all()                 # ... and every cached packed copy is re-made here, in one launch

    def _launch(self, lib, stream, dev):
        es = self.flat_p.element_size()
        rng, ws = self._range_args(lib)
        bufs = self._buffers()
        for i, g in enumerate(self.param_groups):
            row = None if dev is not None else self._row(g, self.steps)
            for lo, hi in g["ranges"]:
                s1, s2 = (None if b is None else b.data_ptr() + lo * es for b in bufs)
                if dev is not None:
                    code = lib.jspsr_optim_step(self.KIND, self.flat_p.data_ptr() + lo * es, self.reducer.flat.data_ptr() + lo * es,
                                                s1, s2, hi - lo, 0.0, 0.0, 0.0, 0.0, 0.0, 0, dev[i].data_ptr(), rng, ws, stream)
                else:
                    code = lib.jspsr_optim_step(self.KIND, self.flat_p.data_ptr() + lo * es, self.reducer.flat.data_ptr() + lo * es,
                                                s1, s2, hi - lo, row[0], row[1], row[2], row[3], row[4], self._step_arg(), None,
                                                rng, ws, stream)
                _lib.check(code, "jspsr_optim_step")

    def _step_arg(self):
        return self.steps

    def zero_grad(self, set_to_none=False):
        self.reducer.zero_grad()

    # -- checkpointing: the reference saves optimizer.state_dict() with every best model (main.py:246-252) and
    #    restores it on resume (utils/utils.py:394) -------------------------------------------------------------------
    def _torch_order(self):
        """The parameters in the order the matching torch optimizer numbers them when built as the reference builds it
        (utils/common_config.py:241-258): model.parameters() order, the `diff_lr` parameters moved to a second group."""
        return [[p for p in self.reducer.params if self._group_of[id(p)] is g] for g in self.param_groups]

    def _has_state(self):
        return bool(self.steps)

    def state_dict(self, layout="flat"):
        """layout="flat" (default): flat state buffers + step count + per-group learning rates; tensors are clones (safe to
        torch.save).  layout="torch": the dict the matching torch.optim class's state_dict() would hold for the same
        parameters (per-parameter state under torch's names, `param_groups` with `params` indices) -- what the reference
        writes into its checkpoints (main.py:246-252) and can resume from (utils/utils.py:394)."""
        name = type(self).__name__
        live = [(n, getattr(self, n, None)) for n in self.STATE]
        live = [(n, b) for n, b in live if b is not None]
        if layout == "torch":
            state, groups, idx = {}, [], 0
            for g, plist in zip(self.param_groups, self._torch_order()):
                ids = []
                for p in plist:
                    off, n = self._slices[id(p)]
                    st = {"step": torch.tensor(float(self.steps))} if self.TORCH_STEP else {}
                    for key, buf in live:
                        st[key] = buf[off:off + n].detach().clone().view_as(p)
                    state[idx] = st
                    ids.append(idx)
                    idx += 1
                groups.append({"lr": g["lr"], "initial_lr": g["initial_lr"], **self._hyper(g), **self._torch_group(g), "params": ids})
            return {"state": state if self._has_state() else {}, "param_groups": groups}
        if layout != "flat":
            raise ValueError(f"{name}.state_dict: layout must be 'flat' or 'torch'")
        return {
            "state": {**{key: buf.detach().clone() for key, buf in live}, "step": int(self.steps), **self._flat_extra()},
            "param_groups": [{"lr": g["lr"], "initial_lr": g["initial_lr"], "ranges": [list(r) for r in g["ranges"]],
                              **self._hyper(g)} for g in self.param_groups],
            "numel": int(self.flat_p.numel()),
        }

    def _flat_extra(self):
        return {}

    def _load_flat_extra(self, state):
        pass

    def _load_groups(self, sd, torch_layout):
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            g["lr"] = float(sg["lr"])
            g["initial_lr"] = float(sg.get("initial_lr", sg["lr"])) if torch_layout else float(sg["initial_lr"])
            for key in ("momentum", "betas"):        # per-group scalars a schedule moves: kept where the group has them
                if key in g and key in sg:
                    g[key] = tuple(sg[key]) if key == "betas" else float(sg[key])
        self._set_hyper(sd["param_groups"][0])

    def load_state_dict(self, sd):
        """In place: the parameters keep aliasing `flat_p`, the gradients keep aliasing the reducer's buffer.  Accepts
        this class's flat layout and the matching torch.optim class's (a checkpoint the reference wrote: per-parameter
        state scattered into the flat buffers in parameter order)."""
        name = type(self).__name__
        if not isinstance(sd, dict) or "param_groups" not in sd or "state" not in sd:
            raise ValueError(f"{name}.load_state_dict: not an optimizer state dict (no 'state' / 'param_groups')")
        if "numel" not in sd:
            if not all("params" in g for g in sd["param_groups"]):
                raise ValueError(f"{name}.load_state_dict: unknown optimizer checkpoint format (neither {name}'s flat "
                                 f"layout nor torch.optim.{self.TORCH_NAME}'s)")
            return self._load_torch(sd)
        if int(sd["numel"]) != self.flat_p.numel() or len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError(f"{name}.load_state_dict: checkpoint was written for a different parameter layout")
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            if [list(r) for r in sg["ranges"]] != [list(r) for r in g["ranges"]]:
                raise ValueError(f"{name}.load_state_dict: parameter-group ranges differ")
        self._load_groups(sd, False)
        for key in self.STATE:
            if key in sd["state"]:
                if getattr(self, key, None) is None:
                    setattr(self, key, torch.zeros_like(self.flat_p))
                getattr(self, key).copy_(sd["state"][key])
            elif getattr(self, key, None) is not None:
                getattr(self, key).zero_()
        self.steps = int(sd["state"]["step"])
        self._load_flat_extra(sd["state"])

    def _load_torch(self, sd):
        name = type(self).__name__
        order = self._torch_order()
        if len(sd["param_groups"]) != len(order) or any(len(g["params"]) != len(pl) for g, pl in zip(sd["param_groups"], order)):
            raise ValueError(f"{name}.load_state_dict: the torch {self.TORCH_NAME} checkpoint groups its parameters differently "
                             f"({[len(g['params']) for g in sd['param_groups']]} vs {[len(pl) for pl in order]}): build the "
                             "optimizer with the same lr_overrides (diff_lr) as the run that wrote it")
        # validate everything first, write afterwards: a checkpoint that is refused leaves the optimizer as it was
        steps, writes, keys = set(), [], set()
        for sg, plist in zip(sd["param_groups"], order):
            for pid, p in zip(sg["params"], plist):
                st = sd["state"].get(pid)
                if st is None:
                    continue                          # torch keeps no state for a parameter that never had a gradient
                for key in self.STATE:
                    t = st.get(key)
                    if t is None:
                        continue                      # (a momentum buffer that was never made)
                    if tuple(t.shape) != tuple(p.shape):
                        raise ValueError(f"{name}.load_state_dict: parameter {pid} has shape {tuple(t.shape)} in the "
                                         f"checkpoint, {tuple(p.shape)} here")
                    keys.add(key)
                writes.append((self._slices[id(p)], st))
                if "step" in st:
                    steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"{name}.load_state_dict: parameters at different step counts {sorted(steps)} (one fused step "
                             "count is kept)")
        first = sd["param_groups"][0]
        for flag in ("amsgrad", "maximize", "centered", "nesterov", "dampening"):
            if first.get(flag):
                raise ValueError(f"{name}.load_state_dict: amsgrad / maximize / centered / nesterov / dampening checkpoints are "
                                 "not supported")
        for key in self.STATE:
            if key in keys and getattr(self, key, None) is None:
                setattr(self, key, torch.zeros_like(self.flat_p))
            if getattr(self, key, None) is not None:
                getattr(self, key).zero_()
        for (off, n), st in writes:
            for key in self.STATE:
                if st.get(key) is not None:
                    getattr(self, key)[off:off + n].copy_(st[key].reshape(-1))
        self._load_groups(sd, True)
        self.steps = steps.pop() if steps else 0
        self._loaded_torch(keys)

    def _loaded_torch(self, keys):
        pass


class FlatAdamW(_FlatOptimizer):
    """lr_overrides: {parameter: lr} -- the reference's optional second parameter group (`diff_lr`: the
    `postprocessor` parameters at lr 3e-4, utils/common_config.py:247-258).  Overridden parameters that are
    neighbours in the flat buffer form one range; a step is one launch per range (2 for the reference's grouping).
    `param_groups` mirrors torch's list of dicts ("lr", "initial_lr") so schedulers can drive it; a group that holds
    "betas" (OneCycleLR writes them) uses its own."""

    KIND = 2                  # JSPSR_OPT_ADAMW
    STATE = ("exp_avg", "exp_avg_sq")
    TORCH_NAME = "AdamW"

    def __init__(self, reducer: GradReducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 lr_overrides=None, _group_extra=None):
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        super().__init__(reducer, lr, lr_overrides, _group_extra)
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)

    def _row(self, g, step):
        import numpy as np
        betas = g.get("betas", self.betas)
        b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))      # the C side raises the float values
        return [g["lr"], betas[0], betas[1], self.eps, self.weight_decay, 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5]

    def _hyper(self, g):
        return {"betas": tuple(g.get("betas", self.betas)), "eps": self.eps, "weight_decay": self.weight_decay}

    def _set_hyper(self, first):
        self.betas, self.eps, self.weight_decay = tuple(first["betas"]), float(first["eps"]), float(first["weight_decay"])

    def _torch_group(self, g):
        return {"amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                "fused": None}

    def _launch(self, lib, stream, dev):
        if self.grad_range is not None or type(self) is not FlatAdamW:
            return super()._launch(lib, stream, dev)
        es = self.flat_p.element_size()          # nothing to monitor: the step this class has always launched
        for i, g in enumerate(self.param_groups):
            betas = g.get("betas", self.betas)
            for lo, hi in g["ranges"]:
                if dev is not None:
                    _lib.check(lib.jspsr_adamw_step_dev(self.flat_p.data_ptr() + lo * es, self.reducer.flat.data_ptr() + lo * es,
                                                        self.exp_avg.data_ptr() + lo * es, self.exp_avg_sq.data_ptr() + lo * es,
                                                        hi - lo, dev[i].data_ptr(), stream), "jspsr_adamw_step_dev")
                else:
                    _lib.check(lib.jspsr_adamw_step(self.flat_p.data_ptr() + lo * es, self.reducer.flat.data_ptr() + lo * es,
                                                    self.exp_avg.data_ptr() + lo * es, self.exp_avg_sq.data_ptr() + lo * es,
                                                    hi - lo, g["lr"], betas[0], betas[1], self.eps,
                                                    self.weight_decay, self.steps, stream), "jspsr_adamw_step")


class FlatAdam(FlatAdamW):
    """torch.optim.Adam over the flat buffers: FlatAdamW with the weight decay coupled (g += wd * p before the moments)."""

    KIND = 1                  # JSPSR_OPT_ADAM
    TORCH_NAME = "Adam"

    def __init__(self, reducer: GradReducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, lr_overrides=None):
        super().__init__(reducer, lr, betas, eps, weight_decay, lr_overrides, {"betas": tuple(betas)})

    def _torch_group(self, g):
        return {**super()._torch_group(g), "decoupled_weight_decay": False}


class _Momentum(_FlatOptimizer):
    """SGD and RMSprop: a momentum buffer that exists only while some group's momentum is not 0, as in torch."""

    def _momentum(self, g):
        return float(g.get("momentum", self.momentum))

    def _ensure_state(self):
        if self.momentum_buffer is None and any(self._momentum(g) != 0.0 for g in self.param_groups):
            self.momentum_buffer = torch.zeros_like(self.flat_p)
            self._buffer_from = self.steps + 1


class FlatSGD(_Momentum):
    """torch.optim.SGD over the flat buffers: momentum >= 0, dampening 0, no Nesterov, coupled weight decay; at the first
    step with momentum the buffer is the gradient itself.  Per-group "momentum" lives in `param_groups` (OneCycleLR
    cycles it)."""

    KIND = 0                  # JSPSR_OPT_SGD
    STATE = ("momentum_buffer",)
    TORCH_STEP = False
    TORCH_NAME = "SGD"

    def __init__(self, reducer: GradReducer, lr=1e-3, momentum=0.0, weight_decay=0.0, lr_overrides=None):
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        super().__init__(reducer, lr, lr_overrides, {"momentum": float(momentum)})
        self.momentum_buffer = None
        self._buffer_from = 0            # the step count at which the buffer is made from the gradient (0: it holds state)
        self._ensure_state()

    def _row(self, g, step):
        return [g["lr"], self._momentum(g), 0.0, 0.0, self.weight_decay, 1.0 if step == self._buffer_from else 0.0, 0.0]

    def _step_arg(self):
        return 1 if self.steps == self._buffer_from else 2

    def _has_state(self):
        return self.momentum_buffer is not None and (self._buffer_from == 0 or self.steps >= self._buffer_from)

    def _hyper(self, g):
        return {"momentum": self._momentum(g), "weight_decay": self.weight_decay}

    def _set_hyper(self, first):
        self.momentum, self.weight_decay = float(first["momentum"]), float(first["weight_decay"])

    def _torch_group(self, g):
        return {"dampening": 0, "nesterov": False, "maximize": False, "foreach": None, "differentiable": False, "fused": None}

    def _flat_extra(self):
        return {"buffer_from": int(self._buffer_from)}

    def _load_flat_extra(self, state):
        self._buffer_from = int(state.get("buffer_from", 0))

    def _loaded_torch(self, keys):
        # torch's SGD keeps no step count: a loaded buffer simply holds state, a missing one is made at the next step
        self._buffer_from = 0 if "momentum_buffer" in keys else 1


class FlatRMSprop(_Momentum):
    """torch.optim.RMSprop over the flat buffers: alpha 0.99, eps 1e-8 added OUTSIDE the square root, not centered,
    coupled weight decay, a momentum buffer only when momentum > 0."""

    KIND = 3                  # JSPSR_OPT_RMSPROP
    STATE = ("square_avg", "momentum_buffer")
    TORCH_NAME = "RMSprop"

    def __init__(self, reducer: GradReducer, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, lr_overrides=None):
        self.alpha, self.eps, self.momentum, self.weight_decay = float(alpha), float(eps), float(momentum), float(weight_decay)
        super().__init__(reducer, lr, lr_overrides, {"momentum": float(momentum)})
        self.square_avg = torch.zeros_like(self.flat_p)
        self.momentum_buffer = None
        self._ensure_state()

    def _row(self, g, step):
        return [g["lr"], self._momentum(g), self.alpha, self.eps, self.weight_decay, 0.0, 0.0]

    def _hyper(self, g):
        return {"momentum": self._momentum(g), "alpha": self.alpha, "eps": self.eps, "weight_decay": self.weight_decay}

    def _set_hyper(self, first):
        self.momentum, self.alpha = float(first["momentum"]), float(first["alpha"])
        self.eps, self.weight_decay = float(first["eps"]), float(first["weight_decay"])

    def _torch_group(self, g):
        return {"centered": False, "capturable": False, "foreach": None, "maximize": False, "differentiable": False}


def tensor_ranges(tensors, table=None):
    """min / max of up to 8 device tensors (fp32 or bf16) in one call (jspsr_tensor_ranges, K11) -> (len(tensors), 4) fp32
    device tensor of rows {min, max, count of non-finite elements, 0}; min / max are over the finite values.  What the
    reference's get_tensor_range (train/train_utils.py:84-96) reads back with .item() per tensor; nothing is read back
    here.  `table`: rows to write into (a contiguous fp32 (len, 4) view) instead of a new tensor."""
    tensors = [t if t.is_contiguous() else t.contiguous() for t in tensors]
    if not 1 <= len(tensors) <= 8:
        raise ValueError(f"tensor_ranges: 1..8 tensors, got {len(tensors)}")
    code = {torch.float32: 0, torch.bfloat16: 1}
    for t in tensors:
        if not t.is_cuda or t.dtype not in code or t.numel() == 0:
            raise ValueError(f"tensor_ranges: non-empty fp32 / bf16 GPU tensors, got {t.dtype} on {t.device} with {t.numel()} elements")
    lib = _lib.load()
    dev = tensors[0].device
    if table is None:
        table = torch.empty((len(tensors), 4), dtype=torch.float32, device=dev)
    elif table.dtype != torch.float32 or tuple(table.shape) != (len(tensors), 4) or not table.is_contiguous() or table.device != dev:
        raise ValueError("tensor_ranges: table must be a contiguous fp32 (len(tensors), 4) tensor on the tensors' device")
    ws = _RANGES_WS.get(dev)
    if ws is None:
        ws = _RANGES_WS[dev] = torch.empty(lib.jspsr_tensor_ranges_workspace_bytes() // 4, dtype=torch.float32, device=dev)
    n = len(tensors)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    numel = (ctypes.c_longlong * n)(*[t.numel() for t in tensors])
    dts = (ctypes.c_int * n)(*[code[t.dtype] for t in tensors])
    _lib.check(lib.jspsr_tensor_ranges(n, ptrs, numel, dts, table.data_ptr(), ws.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "jspsr_tensor_ranges")
    return table


_RANGES_WS = {}


class WarmupStepLR:
    """The reference's "warmupsteplr" schedule (utils/common_config.py:339-358): SequentialLR of
    LambdaLR(1 / 10**(warmup_epoch - e)) for the first `warmup_epoch` epochs, then StepLR(step_size, gamma)
    counted from the hand-over.  Closed form per epoch e (one `step()` per epoch, as train loops call it):

        e <  warmup_epoch :  lr = initial_lr * 10**-(warmup_epoch - e)
        e >= warmup_epoch :  lr = initial_lr * gamma**((e - warmup_epoch) // step_size)

    Works on anything with torch-style `param_groups` (FlatAdamW, torch optimizers)."""

    def __init__(self, optimizer, warmup_epoch=0, step_size=100, gamma=0.5):
        self.optimizer = optimizer
        self.warmup_epoch, self.step_size, self.gamma = int(warmup_epoch), int(step_size), float(gamma)
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.last_epoch = 0
        self._apply()

    def decays(self, epoch: int) -> int:
        """How often StepLR has decayed the rate by `epoch` (>= warmup_epoch)."""
        if self.warmup_epoch == 0:  # SequentialLR never "reaches" a milestone at 0: StepLR then runs one epoch late
            return max(epoch - 1, 0) // self.step_size
        return (epoch - self.warmup_epoch) // self.step_size

    def factor(self, epoch: int) -> float:
        if epoch < self.warmup_epoch:
            return 1.0 / (10.0 ** float(self.warmup_epoch - epoch))
        return self.gamma ** self.decays(epoch)

    def _apply(self):
        e = self.last_epoch
        for g in self.optimizer.param_groups:
            if e < self.warmup_epoch:
                g["lr"] = g["initial_lr"] * self.factor(e)
            else:     # StepLR multiplies the running value by gamma at every decay: the same products, in the same order
                g["lr"] = _decayed(g["initial_lr"], self.gamma, self.decays(e))

    def step(self):
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        self.last_epoch = int(sd["last_epoch"])
        self._apply()


def _decayed(lr, gamma, times):
    """lr after `times` decays as torch's StepLR makes them: one multiplication by gamma each (gamma ** times in one go
    differs from that in the last bit for a gamma like 0.1)."""
    for _ in range(times):
        lr *= gamma
    return lr


class _ClosedFormLR:
    """A schedule as a closed form of the epoch count over torch-style `param_groups` (one `step()` per epoch, as the
    reference's loop calls it, train/train_utils.py:270).  No hidden recursion state: `state_dict()` is {"last_epoch"}
    and a resume is exact.  Works on anything with `param_groups` (the flat optimizers, torch optimizers)."""

    def __init__(self, optimizer):
        self.optimizer = optimizer
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.last_epoch = 0
        self._apply()

    def _set(self, g, epoch):
        raise NotImplementedError

    def _apply(self):
        for g in self.optimizer.param_groups:
            self._set(g, self.last_epoch)

    def step(self):
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        self.last_epoch = int(sd["last_epoch"])
        self._apply()


class OneCycleLR(_ClosedFormLR):
    """torch.optim.lr_scheduler.OneCycleLR with its defaults besides max_lr, total_steps and div_factor: pct_start 0.3,
    cosine anneal, final_div_factor 1e4, two phases, cycle_momentum between 0.85 and 0.95 -- `momentum` of SGD / RMSprop
    groups, `betas[0]` of Adam / AdamW groups (a group that has neither gets "betas" from the optimizer's `betas`).
    As in torch, EVERY group runs from max_lr / div_factor up to max_lr and down to max_lr / (div_factor * 1e4): the
    groups' own learning rates (diff_lr) are overwritten."""

    def __init__(self, optimizer, max_lr, total_steps, div_factor=25.0, pct_start=0.3, final_div_factor=1e4,
                 base_momentum=0.85, max_momentum=0.95):
        if total_steps <= 0:
            raise ValueError(f"OneCycleLR: total_steps must be positive, got {total_steps}")
        self.total_steps = int(total_steps)
        self.max_lr = float(max_lr)
        self.start_lr = self.max_lr / div_factor
        self.min_lr = self.start_lr / final_div_factor
        self.base_momentum, self.max_momentum = float(base_momentum), float(max_momentum)
        self.peak = float(pct_start * self.total_steps) - 1.0
        for g in optimizer.param_groups:
            if "momentum" not in g and "betas" not in g:
                if not hasattr(optimizer, "betas"):
                    raise ValueError("OneCycleLR: the optimizer's groups hold neither 'momentum' nor 'betas'")
                g["betas"] = tuple(optimizer.betas)
            g["initial_lr"] = self.start_lr
        super().__init__(optimizer)

    @staticmethod
    def _cos(start, end, pct):
        return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)

    def _set(self, g, epoch):
        if epoch > self.total_steps:
            raise ValueError(f"OneCycleLR: tried to step {epoch} times, the schedule has {self.total_steps} steps")
        last = float(self.total_steps - 1)
        if epoch <= self.peak:
            pct = epoch / self.peak
            lr, mom = self._cos(self.start_lr, self.max_lr, pct), self._cos(self.max_momentum, self.base_momentum, pct)
        else:
            pct = (epoch - self.peak) / (last - self.peak)
            lr, mom = self._cos(self.max_lr, self.min_lr, pct), self._cos(self.base_momentum, self.max_momentum, pct)
        g["lr"] = lr
        if "betas" in g:
            g["betas"] = (mom, *g["betas"][1:])
        else:
            g["momentum"] = mom


class CosineAnnealingLR(_ClosedFormLR):
    """torch's CosineAnnealingLR in its closed form: eta_min + (initial_lr - eta_min) * (1 + cos(pi * e / T_max)) / 2."""

    def __init__(self, optimizer, T_max, eta_min=0.0):
        self.T_max, self.eta_min = int(T_max), float(eta_min)
        super().__init__(optimizer)

    def _set(self, g, epoch):
        g["lr"] = self.eta_min + (g["initial_lr"] - self.eta_min) * (1 + math.cos(math.pi * epoch / self.T_max)) / 2


class StepLR(_ClosedFormLR):
    """torch's StepLR: initial_lr decayed by gamma e // step_size times."""

    def __init__(self, optimizer, step_size, gamma=0.1):
        self.step_size, self.gamma = int(step_size), float(gamma)
        super().__init__(optimizer)

    def _set(self, g, epoch):
        g["lr"] = _decayed(g["initial_lr"], self.gamma, epoch // self.step_size)


class ConstantLR(_ClosedFormLR):
    """The reference's "constantlr": LambdaLR(lambda x: 1)."""

    def _set(self, g, epoch):
        g["lr"] = g["initial_lr"] * 1


def _get(mapping, key, default=None):
    """p.x / p["x"] / p.get("x") for the reference's EasyDict configs and plain dicts alike."""
    if isinstance(mapping, dict):
        return mapping.get(key, default)
    return getattr(mapping, key, default)


def get_optimizer(p, model, reducer):
    """get_optimizer (utils/common_config.py:241-291) for the flat optimizers.  p: the reference's config (attributes or
    keys): `optimizer` (sgd | adam | adamw | rmsprop, case-insensitive), `optimizer_kwargs` {lr, momentum, weight_decay,
    diff_lr}, `model_name`.  As there, SGD and RMSprop take lr, momentum and weight_decay, Adam and AdamW lr and
    weight_decay; every other setting is torch's default.  diff_lr: JSPSR only -- the named parameters containing
    "postprocessor" at lr 3e-4; any other model raises NotImplementedError.  `reducer` is the GradReducer built over
    model.parameters()."""
    kw = _get(p, "optimizer_kwargs")
    lr, momentum, weight_decay = _get(kw, "lr"), _get(kw, "momentum"), _get(kw, "weight_decay")
    over = None
    if _get(kw, "diff_lr"):
        if "jspsr" in str(_get(p, "model_name")).lower():
            over = {param: 0.0003 for name, param in model.named_parameters() if "postprocessor" in name and param.requires_grad}
        else:
            raise NotImplementedError(f"Undefined model parts for different learning rates: {_get(p, 'model_name')}")
    name = str(_get(p, "optimizer")).lower()
    if name == "sgd":
        return FlatSGD(reducer, lr=lr, momentum=momentum, weight_decay=weight_decay, lr_overrides=over)
    if name == "adam":
        return FlatAdam(reducer, lr=lr, weight_decay=weight_decay, lr_overrides=over)
    if name == "adamw":
        return FlatAdamW(reducer, lr=lr, weight_decay=weight_decay, lr_overrides=over)
    if name == "rmsprop":
        return FlatRMSprop(reducer, lr=lr, momentum=momentum, weight_decay=weight_decay, lr_overrides=over)
    raise NotImplementedError(f"Undefined optimizer: {_get(p, 'optimizer')}")


def get_scheduler(p, optimizer):
    """get_scheduler (utils/common_config.py:294-368).  p: `scheduler` (onecyclelr | cosineannealinglr | steplr |
    warmupsteplr | constantlr, case-insensitive), `epochs`, `scheduler_kwargs` {warmup_epoch 0, max_lr 0.1, step_size
    epochs // 3, gamma 0.1 -- the reference's defaults here, which are not WarmupStepLR's constructor defaults}."""
    kw = _get(p, "scheduler_kwargs") or {}
    epochs = int(_get(p, "epochs"))
    warmup_epoch = _get(kw, "warmup_epoch", 0)
    max_lr = _get(kw, "max_lr", 0.1)
    step_size = _get(kw, "step_size") if _get(kw, "step_size") is not None else epochs // 3
    gamma = _get(kw, "gamma") if _get(kw, "gamma") is not None else 0.1
    name = str(_get(p, "scheduler")).lower()
    if name == "onecyclelr":
        return OneCycleLR(optimizer, max_lr=max_lr, total_steps=epochs, div_factor=90)
    if name == "cosineannealinglr":
        return CosineAnnealingLR(optimizer, T_max=epochs, eta_min=1e-6)
    if name == "steplr":
        return StepLR(optimizer, step_size=step_size, gamma=gamma)
    if name == "warmupsteplr":
        return WarmupStepLR(optimizer, warmup_epoch=warmup_epoch, step_size=step_size, gamma=gamma)
    if name == "constantlr":
        return ConstantLR(optimizer)
    raise NotImplementedError(f"Undefined scheduler: {_get(p, 'scheduler')}")
