"""Restatement of SSIM over a validity plane under the "window" rule (K23: jspsr_loss_menu_valid_ssim_*,
jspsr_ssim_tiles_forward) with autograd, torch CPU only, in the dtype of its operands (fp64 for the reference, fp32 for the
tolerance rule of tests/test_loss_menu_gpu.py::_tolerances).

An element of the SSIM map (tests/loss_menu_ref.ssim_map) counts iff an 11x11 box filter of the INVALID plane -- with the
map's own padding, 0 for the valid map and 5 zeros for the "same" map, so that a padded tap is not a void -- is 0 there.
The operands are replaced by 0 at the invalid pixels before filtering (they have no influence by definition, and a NaN
there would poison autograd's products); the counting rule makes the value independent of that: a counted element reads
valid pixels only.  SSIM = sum_counted S / N_s over the call (the loss: 1 - that, 0 when N_s = 0), or per tile for the
meters (NaN when a tile's N_s = 0).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests import loss_menu_ref as M
from tests import masked_loss_ref as V

SHAPES = [(1, 1, 11, 11), (2, 1, 23, 37), (1, 2, 45, 76), (3, 1, 43, 54)]


def planes(shape, seed=0):
    """name -> (B,1,H,W) bool plane."""
    B, C, H, W = shape
    rs = np.random.RandomState(seed + sum(shape))
    one = np.ones((B, 1, H, W), bool)
    pixel = one.copy()
    pixel[:, :, H // 2, W // 2] = False
    corner = one.copy()
    corner[:, :, 0, 0] = False
    rect = one.copy()
    rect[:, :, : H // 2 + 1, W - 2:] = False
    speckle = rs.rand(B, 1, H, W) >= 0.01
    island = ~one
    y0, x0 = (H - 11) // 2, (W - 11) // 2
    island[0, :, y0:y0 + 11, x0:x0 + 11] = True
    out = dict(ones=one, pixel=pixel, corner=corner, rect=rect, speckle=speckle, island=island, none=~one)
    if B > 1:
        sample = one.copy()
        sample[0] = False
        sample[1:, :, 2, 1] = False
        out["sample"] = sample
    return out


def pair(shape, seed=230):
    """(pred, gt) fp32 torch: DEM-like fields (loss_menu_ref.dem_pair: pred outside [0,1] and on the clamp's edge at a few
    pixels)."""
    p, g = M.dem_pair(seed + sum(shape), shape)
    return torch.from_numpy(p), torch.from_numpy(g)


def expand(valid, like):
    return torch.as_tensor(np.asarray(valid)).bool().expand(like.shape)


def counted_map(v, same=False):
    """(B,C,Hm,Wm) bool from the (B,C,H,W) bool plane: no void under the window (padded taps are not voids)."""
    C = v.shape[1]
    box = torch.ones(C, 1, 11, 11, dtype=torch.float64)
    return F.conv2d((~v).double(), box, padding=5 if same else 0, groups=C) == 0


def ssim_values(x, y, v, window=None, same=False):
    """-> (S zeroed at the uncounted elements, the counted map); x is the CLAMPED prediction."""
    zero = torch.zeros_like(x)
    x, y = torch.where(v, x, zero), torch.where(v, y, zero)
    w = M.gauss1d(dtype=x.dtype) if window is None else window.to(x.dtype)
    s = M.ssim_map(x, y, w, 5 if same else 0, separable=not same)
    c = counted_map(v, same)
    return torch.where(c, s, torch.zeros_like(s)), c


def ssim_loss(pred, gt, v):
    """1 - sum_counted S / N_s over the whole call; 0 when nothing is counted."""
    s, c = ssim_values(pred.clamp(0, 1), gt, v)
    n = int(c.sum())
    if n == 0:
        return s.sum() * 0.0
    return 1 - s.sum() / n


def term(name, p, g, v):
    return ssim_loss(p, g, v) if name.lower() == "ssim" else V.term(name, p, g, v)


def criterion(weights, p, g, v):
    out = {k: term(k, p, g, v) for k in weights}
    out["Total"] = sum(float(w) * out[k] for k, w in weights.items())
    return out


def values_and_grad(weights, pred, gt, valid, up=1.0, dtype=torch.float64):
    """Values {key: float}, d(up * Total)/d(pred) and SSIM's N_s, in `dtype`, on CPU tensors / arrays."""
    p = torch.as_tensor(np.asarray(pred)).to(dtype).clone()
    g = torch.as_tensor(np.asarray(gt)).to(dtype).clone()
    v = expand(valid, p)
    p[~v] = 0.0
    g[~v] = 0.0
    p.requires_grad_()
    out = criterion(dict(weights), p, g, v)
    (up * out["Total"]).backward()
    return {k: float(x.detach()) for k, x in out.items()}, p.grad.clone(), int(counted_map(v).sum())


def tiles(pred, gt, valid, package="piq", border=0.0, window=None, dtype=torch.float64):
    """Per-tile SSIM of uncropped (B,1,H,W) tensors -> ((B,) float64 numpy, NaN where the count is 0; (B,) int counts)."""
    H, W = pred.shape[-2:]
    bh, bw = int(H * border), int(W * border)
    p = torch.as_tensor(np.asarray(pred)).to(dtype)[..., bh:H - bh, bw:W - bw].clamp(0, 1)
    g = torch.as_tensor(np.asarray(gt)).to(dtype)[..., bh:H - bh, bw:W - bw]
    v = torch.ones_like(p, dtype=torch.bool) if valid is None else expand(valid, pred)[..., bh:H - bh, bw:W - bw]
    same = package == "local"
    s, c = ssim_values(p, g, v, window if same else None, same)
    n = c.sum((1, 2, 3))
    vals = torch.where(n > 0, s.sum((1, 2, 3)) / n.clamp_min(1), torch.full((p.shape[0],), float("nan"), dtype=dtype))
    return vals.double().numpy(), n.numpy().astype(np.int64)
