"""fp64 restatement of the masked losses (K19: jspsr_loss_valid_*, jspsr_loss_menu_valid_*) with autograd, torch CPU only.

pred, gt: (B,C,H,W); valid: a bool / uint8 plane of the same shape, or (B,1,H,W) (expanded over C).  With d = pred - gt
and N the number of valid elements of the whole call:
  * the pointwise terms (L1, L2, BerHu, BCE, Norm) by COMPACTION: the term of tests/loss_menu_ref.py over the 1-D tensors
    of the valid elements (BerHu's threshold is then 0.6 max_valid |d|); 0 when nothing is valid;
  * Grad: F.conv2d of the replicate-padded d with the Sobel pair / 8; an output is counted where a 3x3 min-pool of the
    replicate-padded plane is 1 (all nine clamped taps valid); sum_counted (|gx| + |gy|) / (2 N_g), 0 when N_g = 0.  d is
    set to 0 at the invalid pixels BEFORE the convolution so that autograd stays finite whatever the tensors hold there;
    the counting rule makes the value independent of that: a counted output reads valid taps only.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests import loss_menu_ref as M

SOBEL = torch.tensor([[[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]],
                      [[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]]], dtype=torch.float64).unsqueeze(1) / 8.0


def pair(seed, shape):
    """(pred, gt) fp32 numpy of any shape: pred uniform in [0, 1), gt = pred + 0.05 noise, two exact zeros of pred (the
    surface-normal loss's |p| <= eps branch)."""
    rs = np.random.RandomState(seed)
    pred = rs.uniform(0.0, 1.0, shape).astype(np.float32)
    gt = (pred + 0.05 * rs.standard_normal(shape)).astype(np.float32)
    pred[..., 1, 1] = 0.0
    pred[..., shape[2] - 2, shape[3] - 1] = 0.0
    return pred, gt


def plane(valid, like):
    v = torch.as_tensor(np.asarray(valid)).bool()
    return v.expand(like.shape)


def counted(v):
    """(B,C,H,W) bool: the Sobel outputs whose nine replicate-clamped taps are all valid."""
    B, C, H, W = v.shape
    q = F.pad(v.double().reshape(B * C, 1, H, W), (1, 1, 1, 1), mode="replicate")
    return (-F.max_pool2d(-q, 3, stride=1)).reshape(B, C, H, W) == 1


def grad_term(p, g, v):
    B, C, H, W = p.shape
    d = torch.where(v, p - g, torch.zeros_like(p))
    s = F.conv2d(F.pad(d.reshape(B * C, 1, H, W), (1, 1, 1, 1), mode="replicate"), SOBEL).reshape(B, C, 2, H, W)
    c = counted(v)
    n_g = int(c.sum())
    if n_g == 0:
        return d.sum() * 0.0
    return torch.where(c.unsqueeze(2), s.abs(), torch.zeros_like(s)).sum() / (2.0 * n_g)


def pointwise(name, p, g, v):
    if not bool(v.any()):
        return torch.where(v, p, torch.zeros_like(p)).sum() * 0.0
    pc, gc = p[v], g[v]
    if name == "norm":                       # loss_menu_ref.norm sums over dim 1: one channel of N elements
        pc, gc = pc.reshape(-1, 1), gc.reshape(-1, 1)
    return M.TERMS[name](pc, gc)


def term(name, p, g, v):
    name = name.lower()
    if name in ("grad", "edge"):
        return grad_term(p, g, v)
    if name == "ssim":
        raise NotImplementedError("masked SSIM is not built")
    return pointwise(name, p, g, v)


def criterion(weights, p, g, v):
    """{key: term ..., "Total": sum of weight * term} as jspsr_amd.losses.Criterion returns it."""
    out = {k: term(k, p, g, v) for k in weights}
    out["Total"] = sum(float(w) * out[k] for k, w in weights.items())
    return out


def multi_loss(p, g, v, w1=1.0, w2=1.0, wg=0.1):
    return criterion({"L1": w1, "L2": w2, "Grad": wg}, p, g, v)


def values_and_grad(weights, pred, gt, valid, up=1.0):
    """fp64 values {key: float} and d(up * Total)/d(pred) on CPU tensors / arrays; pred and gt at the invalid elements are
    replaced by 0 first (they have no influence by definition, and NaN there would poison autograd's products)."""
    p = torch.as_tensor(np.asarray(pred)).double().clone()
    g = torch.as_tensor(np.asarray(gt)).double().clone()
    v = plane(valid, p)
    p[~v] = 0.0
    g[~v] = 0.0
    p.requires_grad_()
    out = criterion(dict(weights), p, g, v)
    (up * out["Total"]).backward()
    return {k: float(x.detach()) for k, x in out.items()}, p.grad.clone()
