"""Training loss of the reference configs (configs/*.yml:67-70): L1 + L2 + 0.1 * Sobel-L1
(losses/loss_schemes.py:55-72, losses/loss_functions.py:171-185) as one fused HIP forward and one
fused HIP backward over the (B,1,H,W) prediction (jspsr_loss_forward / jspsr_loss_backward).

The rest of the reference's loss menu -- every name `get_loss` accepts (loss_schemes.py:6-33) -- and the criterion
`get_criterion` builds from a config's `loss:` dict (utils/common_config.py:209-233) run on the device too
(jspsr_loss_menu_forward / _backward, csrc/loss_terms.hip): one fused forward and one fused backward for the whole dict.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


# The C entries without and with a validity plane: (the fused L1 + L2 + Grad pair, the menu).  A masked call passes the
# plane after gt, and the menu its SSIM rule after W; everything else is one argument list.  jspsr_loss_menu_valid_* is the
# _valid_ssim_ family with the SSIM bit refused, so the menu never calls it.
_ENTRY = {False: ("jspsr_loss", "jspsr_loss_menu"), True: ("jspsr_loss_valid", "jspsr_loss_menu_valid_ssim")}


def _call(stem, what, *args):
    name = f"{stem}_{what}"
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _check_pair(pred, gt):
    if not pred.is_cuda:
        raise RuntimeError("jspsr_amd losses run on the GPU only (no CPU fallback)")
    if pred.shape != gt.shape or pred.dim() != 4:
        raise ValueError(f"loss: expected equal (B,C,H,W) shapes, got {tuple(pred.shape)} {tuple(gt.shape)}")


def _fused_forward(pred, gt, valid, weights):
    """jspsr_loss[_valid]_forward on contiguous fp32 (B,C,H,W) -> (losses[4], workspace)."""
    B, C, H, W = pred.shape
    stem = _ENTRY[valid is not None][0]
    plane = () if valid is None else (valid.data_ptr(),)
    ws = torch.empty(getattr(_lib.load(), stem + "_workspace_bytes")(B * C, H, W), dtype=torch.uint8, device=pred.device)
    losses = torch.empty(4, dtype=torch.float32, device=pred.device)
    _call(stem, "forward", pred.data_ptr(), gt.data_ptr(), *plane, *weights, losses.data_ptr(), ws.data_ptr(), B * C, H, W,
          _stream())
    return losses, ws


def _fused_backward(pred, gt, valid, weights, g, ws):
    """jspsr_loss[_valid]_backward: writes every element of the gradient (+0.0 at the invalid ones); g: d/d(Total), (1,)."""
    B, C, H, W = pred.shape
    plane = () if valid is None else (valid.data_ptr(),)
    gp = torch.empty_like(pred)
    _call(_ENTRY[valid is not None][0], "backward", pred.data_ptr(), gt.data_ptr(), *plane, g.data_ptr(), *weights,
          gp.data_ptr(), ws.data_ptr(), B * C, H, W, _stream())
    return gp


class _FusedLoss(torch.autograd.Function):
    """losses = (L1, L2, Grad, Total), over the elements `valid` keeps (K19) or, valid None, over all."""

    @staticmethod
    def forward(ctx, pred, gt, valid, w1, w2, wg):
        pred_c, gt_c = pred.float().contiguous(), gt.float().contiguous()
        losses, ws = _fused_forward(pred_c, gt_c, valid, (w1, w2, wg))
        ctx.save_for_backward(pred_c, gt_c, valid, ws)
        ctx.w = (w1, w2, wg)
        ctx.mark_non_differentiable(gt)
        return losses

    @staticmethod
    def backward(ctx, glosses):
        pred, gt, valid, ws = ctx.saved_tensors
        # only "Total" carries gradient (MultiLoss detaches the three components)
        g = glosses.float().contiguous()[3:4].contiguous()
        return _fused_backward(pred, gt, valid, ctx.w, g, ws), None, None, None, None, None


def _plane(pred, valid):
    """The validity plane of a masked call as contiguous (B,C,H,W) bytes: (B,1,H,W) or (B,C,H,W), uint8 or bool, on pred's
    device; nonzero = valid.  Raised before any launch: TypeError for another dtype, ValueError for another shape."""
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"loss: valid must be a uint8 or bool tensor, got {getattr(valid, 'dtype', type(valid).__name__)}")
    B, C, H, W = pred.shape
    if valid.dim() != 4 or tuple(valid.shape) not in {(B, 1, H, W), (B, C, H, W)}:
        raise ValueError(f"loss: valid must be (B,1,H,W) or (B,C,H,W) of pred {tuple(pred.shape)}, got {tuple(valid.shape)}")
    if valid.device != pred.device:
        raise ValueError(f"loss: valid is on {valid.device}, pred on {pred.device}")
    if valid.dtype == torch.bool:
        valid = valid.view(torch.uint8)
    return valid.expand(B, C, H, W).contiguous()


def _fused(pred, gt, valid, weights):
    """The fused L1 + L2 + Grad pair, unmasked (valid None) or over a validity plane."""
    _check_pair(pred, gt)
    return _FusedLoss.apply(pred, gt, None if valid is None else _plane(pred, valid), *weights)


class MultiLoss(torch.nn.Module):
    """Returns the reference's dict {"L1","L2","Grad","Total"} (loss_schemes.py:61-72).  Gradients flow
    through "Total" (what the reference back-propagates, train/train_utils.py:217)."""

    def __init__(self, l1=1.0, l2=1.0, grad=0.1):
        super().__init__()
        self.weights = (float(l1), float(l2), float(grad))
        self.out = {}

    def forward(self, pred, gt, valid=None):
        """valid: None, or the plane of the elements that count ((B,1,H,W) or (B,C,H,W), uint8 or bool, on the device; see
        `Criterion`): a masked element has no influence, whatever pred and gt hold there."""
        v = _fused(pred, gt, valid, self.weights)
        self.out = {"L1": v[0].detach(), "L2": v[1].detach(), "Grad": v[2].detach(), "Total": v[3]}
        return self.out

    def reset(self):
        """The reference's train loop calls criterion.reset() every iteration (train/train_utils.py:206;
        loss_schemes.py:74-75)."""
        self.out = {}

    def __str__(self):
        return f"{self.__class__.__name__}:: ['L1', 'L2', 'Grad'], {list(self.weights)}, fused HIP (jspsr_loss_forward/backward)"


# ---- the loss menu -------------------------------------------------------------------------------------------------
# get_loss's names and aliases (case-insensitive) -> term slot of jspsr_loss_menu_*: 0..2 are the three terms of
# jspsr_loss_forward, 3..6 the terms of csrc/loss_terms.hip (bit 1 << (slot - 3) of its `terms` set)
_SLOT = {"l1": 0, "l2": 1, "mse": 1, "edge": 2, "grad": 2, "berhu": 3, "vanilla": 4, "bce": 4, "norm": 5, "ssim": 6}
_NSLOT = 7


def _slot(name):
    s = _SLOT.get(str(name).lower())
    if s is None:
        raise NotImplementedError(f"Undefined loss: {name}")
    return s


SSIM_RULES = {"window": 1}      # ssim_valid -> ssim_rule of jspsr_loss_menu_valid_ssim_*


class _Spec:
    """Host-side plan of one criterion: keys in config order, their slots and weights, the per-slot weight sums, and the
    rule SSIM follows over a validity plane (None: not accepted)."""

    def __init__(self, weights, ssim_valid=None):
        if ssim_valid is not None and ssim_valid not in SSIM_RULES:
            raise ValueError(f"loss: ssim_valid must be None or one of {sorted(SSIM_RULES)}, got {ssim_valid!r}")
        self.ssim_valid = ssim_valid
        self.keys = list(weights)
        self.slots = [_slot(k) for k in self.keys]
        self.weights = [float(weights[k]) for k in self.keys]
        self.slot_w = [0.0] * _NSLOT
        for s, w in zip(self.slots, self.weights):
            self.slot_w[s] += w
        self.terms = sum(1 << (s - 3) for s in set(self.slots) if s >= 3)
        self.base = any(s < 3 for s in self.slots)
        self.base_w = tuple(self.slot_w[:3])
        n = len(self.keys)
        self.c_slots = (ctypes.c_int * n)(*self.slots)
        self.c_weights = (ctypes.c_double * n)(*self.weights)
        self.c_slot_w = (ctypes.c_double * _NSLOT)(*self.slot_w)

    def check(self, pred, gt):
        """Shape rules, raised before any launch."""
        _check_pair(pred, gt)
        if 5 in self.slots and pred.shape[1] != 1:
            raise ValueError(f"loss Norm: supported for one channel (the DEM head) only, got C = {pred.shape[1]}")
        if 6 in self.slots and (pred.shape[2] < 11 or pred.shape[3] < 11):
            raise ValueError(f"loss SSIM: needs H, W >= 11 (11x11 window, valid map), got {tuple(pred.shape[2:])}")


class _MenuLoss(torch.autograd.Function):
    """out = (term of every key in config order..., Total), over the elements `valid` keeps (K19; SSIM under spec's rule,
    K23) or, valid None, over all.  Only Total carries gradient."""

    @staticmethod
    def forward(ctx, pred, gt, valid, spec):
        pred_c, gt_c = pred.float().contiguous(), gt.float().contiguous()
        B, C, H, W = pred_c.shape
        P = B * C
        stem = _ENTRY[valid is not None][1]
        # the C side ignores the rule without the SSIM bit, except for its range check: 1 then
        plane, rule = ((), ()) if valid is None else ((valid.data_ptr(),), (SSIM_RULES.get(spec.ssim_valid, 1),))
        base, bws = _fused_forward(pred_c, gt_c, valid, spec.base_w) if spec.base else (None, None)
        ws = torch.empty(getattr(_lib.load(), stem + "_workspace_bytes")(spec.terms, P, H, W, *rule), dtype=torch.uint8,
                         device=pred.device)
        out = torch.empty(len(spec.keys) + 1, dtype=torch.float32, device=pred.device)
        _call(stem, "forward", pred_c.data_ptr(), gt_c.data_ptr(), *plane, spec.terms, P, H, W, *rule, len(spec.keys),
              spec.c_slots, spec.c_weights, base.data_ptr() if base is not None else None, out.data_ptr(), ws.data_ptr(),
              _stream())
        ctx.save_for_backward(pred_c, gt_c, valid, ws, bws)
        ctx.spec = spec
        ctx.mark_non_differentiable(gt)
        return out

    @staticmethod
    def backward(ctx, gout):
        pred, gt, valid, ws, bws = ctx.saved_tensors
        spec = ctx.spec
        B, C, H, W = pred.shape
        n = len(spec.keys)
        g = gout[n:n + 1].float().contiguous()
        plane, rule = ((), ()) if valid is None else ((valid.data_ptr(),), (SSIM_RULES.get(spec.ssim_valid, 1),))
        # the fused pair writes the gradient of the L1 / L2 / Grad part (+0.0 at the invalid elements); the menu adds its
        # own terms at the valid ones
        gp = _fused_backward(pred, gt, valid, spec.base_w, g, bws) if spec.base else torch.zeros_like(pred)
        _call(_ENTRY[valid is not None][1], "backward", pred.data_ptr(), gt.data_ptr(), *plane, spec.terms, B * C, H, W, *rule,
              spec.c_slot_w, g.data_ptr(), gp.data_ptr(), ws.data_ptr(), _stream())
        return gp, None, None, None


def _evaluate(spec, pred, gt, valid=None):
    """-> (components in config order, Total): one fused forward, one fused backward.  valid: the plane of the elements
    that count, or None."""
    spec.check(pred, gt)
    n = len(spec.keys)
    if valid is not None:
        if 6 in spec.slots and spec.ssim_valid is None:
            raise NotImplementedError("loss SSIM: a validity plane is not built (an 11x11-window validity rule is a feature "
                                      "of its own); drop SSIM from the criterion or pass valid=None")
        valid = _plane(pred, valid)
    if spec.terms == 0:      # L1 / L2 / Grad (any aliases) only: exactly the fused pair MultiLoss runs
        v = _FusedLoss.apply(pred, gt, valid, *spec.base_w)
        return [v[s].detach() for s in spec.slots], v[3]
    v = _MenuLoss.apply(pred, gt, valid, spec)
    return [v[i].detach() for i in range(n)], v[n]



class LossTerm(torch.nn.Module):
    """One term of the menu on its own, like the module the reference's get_loss returns: (pred, gt) -> 0-d tensor."""

    def __init__(self, name, ssim_valid=None):
        super().__init__()
        self.name = str(name)
        self.spec = _Spec({self.name: 1.0}, ssim_valid)

    def forward(self, pred, gt, valid=None):
        return _evaluate(self.spec, pred, gt, valid)[1]

    def __str__(self):
        return f"{self.__class__.__name__}({self.name}), fused HIP"


def get_loss(name, ssim_valid=None):
    """The reference's get_loss (losses/loss_schemes.py:6-33) on the device: l1, l2 / mse, vanilla / bce, edge / grad,
    berhu, norm, ssim, case-insensitively.

    Semantics and where they depart from the reference:
      * berhu: th = 0.6 * max|pred - gt| (double from the fp32 max, as `.item()` gives it), compared in fp32, th^2 and
        2 th rounded to fp32; the gradient treats th as a constant.  It stays on the device (the reference's `.item()`
        is a host sync).  At pred == gt everywhere (th = 0) the loss is 0 and the gradient is 0; the reference's
        gradient there is NaN (its unselected torch.where branch divides by 0).
      * norm: F.normalize over the channel of a ONE-channel map (the DEM head); ValueError for C != 1.  Its gradient is
        0 where |pred| > 1e-12 (the reference's autograd leaves residues of about 2e-16 there) and -g^/(1e-12 N) below.
      * bce: max(x, 0) - x y + log1p(exp(-|x|)), gradient (sigmoid(x) - y) / N.
      * ssim: 1 - piq.ssim(clamp(pred, 0, 1), gt, data_range=1, reduction="mean", downsample=False) -- restated from
        piq's public source, UNPINNED against piq itself (not installed here): valid 11x11 Gaussian window (sigma 1.5),
        c1 = 0.01^2, c2 = 0.03^2, the mean of the map over every element of every plane.  piq's input-range assertion
        (a host sync) is not reproduced.  ValueError for H or W < 11.
    Unknown names raise NotImplementedError("Undefined loss: <name>").
    ssim_valid: the rule SSIM follows when the call is given a validity plane (see `Criterion`); None refuses one."""
    _slot(name)
    return LossTerm(name, ssim_valid)


class Criterion(torch.nn.Module):
    """get_criterion's criterion on the device: the components (detached device scalars, keys in the config's spelling
    and order) and "Total" (what carries gradient, train/train_utils.py:214-226).  One fused forward and one fused
    backward for the whole dict; no host synchronisation, so GraphedStep can capture it.

    forward(pred, gt, valid=None) -- valid (K19): the plane of the elements that count, (B,1,H,W) or (B,C,H,W), uint8 or
    bool, on the device (a batch's `batch["valid"]`); a (B,1,H,W) plane is expanded over C here.  A masked element has no
    influence whatever pred and gt hold there, and its gradient is +0.0.  With d = pred - gt and N the valid elements of the
    whole call: L1, L2, BerHu (th = 0.6 max_valid |d|), BCE and Norm sum over the valid elements and divide by N; a Sobel
    output counts iff its nine replicate-clamped taps are valid, Grad = sum_counted (|gx| + |gy|) / (2 N_g).  N = 0 or N_g =
    0 gives value and gradient 0, not NaN.  N and N_g stay on the device, so the masked pair captures in a graph as well.
    An all-ones plane gives the bits of valid=None.  SSIM with a plane raises NotImplementedError before any launch,
    unless the criterion was built with ssim_valid="window" (K23; any other value but None is a ValueError here): an
    element of the (H-10) x (W-10) SSIM map then counts iff all 121 pixels under its window are valid, SSIM = 1 -
    sum_counted S / N_s over the counted elements of the whole call, 0 (and gradient 0) when N_s = 0; N_s stays on the
    device as well, and the all-ones plane still gives the bits of valid=None.  ssim_valid changes nothing without a plane."""

    def __init__(self, weights, single=False, ssim_valid=None):
        super().__init__()
        if not weights:
            raise ValueError("get_criterion: empty loss config")
        self.single = single
        self.spec = _Spec(weights, ssim_valid)
        self.out = {}

    def forward(self, pred, gt, valid=None):
        comps, total = _evaluate(self.spec, pred, gt, valid)
        self.out = dict(zip(self.spec.keys, comps))
        self.out.pop("Total", None)
        self.out["Total"] = total
        return self.out

    def reset(self):
        self.out = {}

    def __str__(self):
        if self.single:
            return f"SingleLoss:: {self.spec.keys[0]}:: fused HIP (jspsr_loss_menu_forward/backward)"
        return f"MultiLoss:: {self.spec.keys}, {self.spec.weights}, fused HIP (jspsr_loss_menu_forward/backward)"


def get_criterion(config, ssim_valid=None):
    """utils/common_config.py:209-233: one key -> that term alone with weight 1 (whatever the configured weight),
    returning {name: v, "Total": v}; several keys -> the weighted sum, {keys in config order..., "Total"}.
    The default {"L1": 1, "L2": 1, "Grad": 0.1} runs exactly MultiLoss(1, 1, 0.1)'s fused pair.
    ssim_valid: passed to `Criterion` ("window": SSIM accepts a validity plane)."""
    config = dict(config)
    if len(config) == 1:
        (name, _), = config.items()
        return Criterion({name: 1.0}, single=True, ssim_valid=ssim_valid)
    return Criterion(config, ssim_valid=ssim_valid)
