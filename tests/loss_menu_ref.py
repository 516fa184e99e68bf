"""fp64 restatements of the loss menu (losses/loss_schemes.py:6-33 get_loss; losses/loss_functions.py:191-239 BerHu,
surface normal, SSIM; evaluation/metrics.py:20-63 the local ssim) and the seeded inputs of tests/golden/g10_loss_menu.npz
(tools/gen_golden_losses.py).  torch CPU only; the GPU tests compare jspsr_amd's kernels against these.

piq's SSIM (SSIMLoss = 1 - piq.ssim(pred.clamp(0,1), gt, data_range=1, reduction="mean", downsample=False)) is restated
from piq's public source and is UNPINNED against piq, which is not installed here: 11-tap Gaussian (sigma 1.5,
normalised, 2-D window = outer product), valid convolution, c1 = 0.01^2, c2 = 0.03^2, per-plane spatial mean then the
mean over planes and batch, no downsampling.  The closest pin is `ssim_map` run with the reference's own local window and
zero padding, which reproduces the reference's local ssim."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

SEED = 2610
SHAPE = (2, 1, 24, 29)
SSIM_SHAPES = ((1, 1, 23, 37), (2, 1, 17, 30))      # the local-ssim fixtures: odd shapes, not multiples of a tile
C1, C2 = 0.01 ** 2, 0.03 ** 2


def dem_pair(seed, shape):
    """(pred, gt) fp32 numpy: smooth DEM-like fields in [0,1] plus noise, a flat patch, pred outside [0,1] at a few
    pixels and exact zeros of pred (the surface-normal loss's |p| <= eps branch)."""
    rs = np.random.RandomState(seed)
    B, C, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64) / max(H, W)
    gt = np.empty(shape)
    for b in range(B):
        for c in range(C):
            a, f, ph = rs.uniform(0.3, 0.6), rs.uniform(2.0, 6.0), rs.uniform(0.0, 2 * math.pi)
            gt[b, c] = a + 0.2 * np.sin(f * xx + ph) * np.cos(0.7 * f * yy + ph) + 0.1 * yy
    pred = gt + rs.normal(0.0, 0.04, shape)
    gt[..., 2:7, 3:11] = 0.45                              # flat region
    pred[..., 2:7, 3:11] = 0.45 + rs.normal(0.0, 0.002, (B, C, 5, 8))
    pred[..., H - 2, 1], pred[..., 1, W - 3] = 1.25, -0.15  # outside [0,1]
    pred[..., H // 2, W // 2] = 1.0                         # on the clamp's edge
    pred[..., 3, 5] = 0.0                                   # exact zeros
    pred[..., H - 4, W - 6] = 0.0
    return pred.astype(np.float32), gt.astype(np.float32)


def inputs(seed=SEED, shape=SHAPE):
    return dem_pair(seed, shape)


def ssim_inputs(i):
    p, g = dem_pair(SEED + 1 + i, SSIM_SHAPES[i])
    return np.clip(p, 0.0, 1.0), g                          # prepared tiles (MeterBase._prepare clamps the prediction)


def checksum(arrays):
    return float(sum(np.asarray(a, dtype=np.float64).sum() * (i + 1) + np.abs(np.asarray(a, dtype=np.float64)).sum()
                     for i, a in enumerate(arrays)))


# ---- pointwise terms ------------------------------------------------------------------------------------------------
def l1(p, g):
    return (p - g).abs().mean()


def l2(p, g):
    return ((p - g) ** 2).mean()


def bce(x, y):
    """max(x, 0) - x y + log1p(exp(-|x|)), written per branch so that autograd gives sigmoid(x) - y at x = 0 too."""
    return (torch.where(x >= 0, x + torch.log1p(torch.exp(-x)), torch.log1p(torch.exp(x))) - x * y).mean()


def berhu(p, g):
    """th = 0.6 max|d| as a constant; at th = 0 the |d| branch alone (zero gradient; the reference's is NaN)."""
    diff = (p - g).abs()
    th = 0.6 * diff.max().item()
    if th == 0:
        return diff.mean()
    return torch.where(diff <= th, diff, (diff ** 2 + th ** 2) / (2 * th)).mean()


def norm(p, g, eps=1e-12):
    """F.normalize over dim 1 (one channel) of both, 1 - <p^, g^>, mean."""
    pn = p / p.abs().clamp_min(eps)
    gn = g / g.abs().clamp_min(eps)
    return (1 - (pn * gn).sum(1)).mean()


def norm_grad(p, g, eps=1e-12):
    """The analytic gradient of `norm` for C = 1: 0 where |p| > eps, -g^/(eps N) where |p| <= eps."""
    gn = g / g.abs().clamp_min(eps)
    return torch.where(p.abs() <= eps, -gn / (eps * p.numel()), torch.zeros_like(p))


# ---- SSIM -------------------------------------------------------------------------------------------------------------
def gauss1d(size=11, sigma=1.5, dtype=torch.float64):
    c = torch.arange(size, dtype=dtype) - (size - 1) / 2.0
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def ssim_map(x, y, w1d, pad, separable=True):
    """The SSIM map with window w1d (x) w1d (2-D window = outer product), zero padding `pad` (0 = valid)."""
    C, k = x.shape[1], w1d.numel()
    w1d = w1d.to(x.dtype)

    def filt(t):
        if separable:
            t = F.conv2d(t, w1d.view(1, 1, 1, k).expand(C, 1, 1, k), padding=(0, pad), groups=C)
            return F.conv2d(t, w1d.view(1, 1, k, 1).expand(C, 1, k, 1), padding=(pad, 0), groups=C)
        return F.conv2d(t, torch.outer(w1d, w1d).view(1, 1, k, k).expand(C, 1, k, k), padding=pad, groups=C)

    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def ssim_piq(x, y, separable=True):
    """piq.ssim(x, y, data_range=1, reduction="mean", downsample=False)."""
    return ssim_map(x, y, gauss1d(dtype=x.dtype), 0, separable).mean()


def ssim_loss(pred, gt):
    """SSIMLoss: 1 - piq.ssim(pred.clamp(0, 1), gt)."""
    return 1 - ssim_piq(pred.clamp(0, 1), gt)


def ssim_local(img1, img2, window):
    """The reference's local ssim(img1, img2) (metrics.py:20-63): 2-D window outer(window), zero padding 5."""
    return ssim_map(img1, img2, window, 5, separable=False).mean()


TERMS = {"l1": l1, "l2": l2, "mse": l2, "bce": bce, "vanilla": bce, "berhu": berhu, "norm": norm, "ssim": ssim_loss}


def value_and_grad(fn, pred, gt):
    """fp64 value and d/d(pred) of fn(pred, gt) on CPU tensors / arrays."""
    p = torch.as_tensor(np.asarray(pred)).double().clone().requires_grad_()
    g = torch.as_tensor(np.asarray(gt)).double()
    v = fn(p, g)
    v.backward()
    return v.item(), p.grad.clone()
