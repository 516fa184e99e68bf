"""Plain torch restatement of ONE general propagation step (K1s, csrc/prop_steps.hip) and the seeded inputs of
tests/test_prop_steps_gpu.py.  CPU only, generic in dtype: the tests hold the kernels to the fp64 evaluation and take
their tolerance from the fp32 evaluation of the very same expressions.

    out = b0 + sum_k wk[k] * (a_k - [normalize] * mean_k a) * S_k + scale * dem

S_k is the deformable 3x3 sampler of oracle/jspsr_ref.py (`sample_taps`, formulation A: explicit 4-corner gather, corners
outside the raster read as 0), the gradients are autograd's.  A non-finite sampling offset means "outside the raster"
to the kernel (prop_tile.h, corners_fast); `sample_taps` would carry the NaN of `inf - floor(inf)` into the backward, so
such offsets are moved to a far finite position here first (their own gradient is then 0, as the kernel's is).
"""
from __future__ import annotations

import torch

from oracle import jspsr_ref as R

CENTRE = (8, 9)            # the centre tap's (dy, dx) channels of the 18-channel offset layout
FAR = 1.0e6                # stands for a non-finite offset: no corner inside any raster


def to18(off):
    """(B,16,H,W) -> (B,18,H,W) with a zero centre pair; an 18-channel tensor is returned as it is."""
    if off.shape[1] == 18:
        return off
    z = torch.zeros_like(off[:, :2])
    return torch.cat((off[:, :8], z, off[:, 8:]), 1)


def to16(off18):
    return torch.cat((off18[:, :8], off18[:, 10:]), 1)


def step(dem, weight, offset, wk, b0, scale, normalize):
    """One step in the dtype of its operands.  offset (B,16|18,H,W); wk 9 values; b0 1 value."""
    off = to18(offset)
    off = torch.where(torch.isfinite(off), off, torch.full_like(off, FAR))
    S = R.sample_taps(dem, off)
    m = weight - weight.mean(1, keepdim=True) if normalize else weight
    return b0.reshape(1, 1, 1, 1) + (wk.reshape(1, 9, 1, 1) * m * S).sum(1, keepdim=True) + scale * dem


def step_grads(dem, weight, offset, wk, b0, scale, normalize, gout, dtype=torch.float64):
    """-> dict(out, grad_weight, grad_offset, grad_dem, grad_wk, grad_b0) of one step evaluated in `dtype` (autograd
    with `gout` as the incoming gradient).  grad_offset has the channel count of `offset`."""
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in (dem, weight, offset, wk.reshape(-1), b0.reshape(-1))]
    out = step(*leaves, scale, normalize)
    gd, gw, go, gk, gb = torch.autograd.grad(out, leaves, gout.to(dtype))
    return dict(out=out.detach(), grad_weight=gw, grad_offset=go, grad_dem=gd, grad_wk=gk, grad_b0=gb)


def smooth_mask(offset, H, W, eps=1e-4):
    """True where d/d(offset) is compared: both sampling coordinates of the tap further than `eps` from an integer (the
    derivative of a bilinear sample jumps there and the kernel's fp32 coordinate may sit on the other side), the centre
    pair of the 18-channel layout excluded by name.  Non-finite coordinates count as kinks.  Same shape as `offset`."""
    off = to18(offset).double()
    B = off.shape[0]
    ys = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    ky = torch.tensor([k // 3 - 1 for k in range(9)], dtype=torch.float64).view(1, 9, 1, 1)
    kx = torch.tensor([k % 3 - 1 for k in range(9)], dtype=torch.float64).view(1, 9, 1, 1)
    pos = off.reshape(B, 9, 2, H, W).clone()
    pos[:, :, 0] += ys + ky
    pos[:, :, 1] += xs + kx
    frac = (pos - pos.round()).abs()
    ok = (frac > eps).all(2, keepdim=True).expand(B, 9, 2, H, W).reshape(B, 18, H, W).clone()
    ok[:, CENTRE[0]:CENTRE[1] + 1] = False
    return ok if offset.shape[1] == 18 else to16(ok)


def non_centre(offset):
    """Number of offset entries outside the centre pair (the denominator of the mask's drop rate)."""
    B, oc, H, W = offset.shape
    return B * 16 * H * W


def case(B, H, W, oc, seed, sigma=2.0, clamp=6.5):
    """Seeded fp32 operands of one step: a white-noise raster in [0, 0.5), grad_out ~ N(0,1), affinities in (0,1), offsets
    sigma * N(0,1) clamped to +-clamp px (no tap leaves tile + halo), tap weights around 1, a bias.  (The raster's
    amplitude sets the slope that turns an fp32 coordinate's rounding into a value error.  At amplitude 1 the fp32
    evaluation's OWN grad_wk error at 3 x 45 x 200 -- 27 000 such errors summed -- is 2.0e-4, and 4 x that is past the
    5e-4 the tests allow a derived tolerance to reach; at 0.5 every quantity at every shape stays inside.)"""
    g = torch.Generator().manual_seed(seed)
    dem = 0.5 * torch.rand(B, 1, H, W, generator=g)
    weight = torch.rand(B, 9, H, W, generator=g)
    off = sigma * torch.randn(B, 18, H, W, generator=g)
    if clamp is not None:
        off = off.clamp(-clamp, clamp)
    off[:, CENTRE[0]:CENTRE[1] + 1] = 0
    wk = 1 + 0.3 * torch.randn(9, generator=g)
    b0 = 0.1 * torch.randn(1, generator=g)
    gout = torch.randn(B, 1, H, W, generator=g)
    return dict(dem=dem, weight=weight, offset=off if oc == 18 else to16(off), wk=wk, b0=b0, gout=gout)
