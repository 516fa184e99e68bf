"""Evaluation scores of the reference, computed where the prediction lives (no host round trip per
sample): PSNR, RMSE, median error, NMAD, LE95 on de-scaled elevations.

Restates evaluation/metrics.py: ``MeterBase._prepare`` :147-199 (border crop by a fraction of the
size, clamp of the prediction to [0,1]); PSNR :229-235 (piq.psnr(data_range=1, reduction="mean"):
10*log10(1 / (mse + 1e-8)) per sample -- epsilon recalled from piq's public source, unpinned);
RMSE :361-384; median :444-455; NMAD :499-512 (1.4826 * median|dh - median dh|); LE95 :556-570
(k-th smallest |dh| with k = 1 + round(0.95 (n-1))), and data/data_utils.py:441-457
``ToDEM.descale_data`` / :289-312 ``ToTensor.scale_data``.  The reference feeds batches of one tile.
SSIM (MeterSSIM :275-335, opt-in): packages "piq" and "local" (``ssim``).
``batch_scores`` gives the scores of a whole batch of tiles in one launch, with the local PSNR (:97-113) and the slope
score (MeterSlope :595-688, "local" and "kornia") beside the five above; ``jspsr_amd.evaluate`` builds the validation
pass on it.
"""
from __future__ import annotations

import ctypes
from math import exp, log

import torch

from . import _lib


def _elev_hip(t, descale, elev_min, elev_max, elev_log, base_elev=0.0):
    """fp32 device rasters: one HIP pass (csrc/tiles.hip, jspsr_elev_scale_f32)."""
    t = t.contiguous()
    out = torch.empty_like(t)
    _lib.check(_lib.load().jspsr_elev_scale_f32(t.data_ptr(), out.data_ptr(), t.numel(), int(descale), int(bool(elev_log)), float(elev_min),
                                                float(elev_max), float(base_elev), torch.cuda.current_stream().cuda_stream),
               "jspsr_elev_scale_f32")
    return out


def scale_data(z, elev_min, elev_max, elev_log=False, base_elev=0.0):
    """metres -> network range (data_utils.py:289-312)."""
    if z.is_cuda and z.dtype == torch.float32 and z.numel() and not z.requires_grad:
        return _elev_hip(z, False, elev_min, elev_max, elev_log, base_elev)
    z = z - base_elev if base_elev != 0 else z
    if elev_log:
        return torch.log(z - elev_min) / log(elev_max - elev_min) + 1e-8
    return (z - elev_min) / (elev_max - elev_min)


def descale_data(v, elev_min, elev_max, elev_log=False):
    """network range -> metres (data_utils.py:441-457)."""
    if v.is_cuda and v.dtype == torch.float32 and v.numel() and not v.requires_grad:
        return _elev_hip(v, True, elev_min, elev_max, elev_log)
    if elev_log:
        return torch.exp(v * log(elev_max - elev_min)) + elev_min
    return v * (elev_max - elev_min) + elev_min


def prepare(pred, gt, border=0.0):
    """metrics.py:147-199: crop `border` (fraction) on every side, clamp the prediction to [0,1]."""
    assert pred.shape == gt.shape, f"{pred.shape} {gt.shape}"
    if border != 0:
        h, w = pred.shape[-2:]
        bh, bw = int(h * border), int(w * border)
        pred, gt = pred[..., bh:h - bh, bw:w - bw], gt[..., bh:h - bh, bw:w - bw]
    return pred.clamp(0.0, 1.0), gt


def psnr(pred, gt):
    """piq.psnr(gt, pred, data_range=1, reduction='mean') on [0,1] tensors (B,1,H,W)."""
    mse = ((pred - gt) ** 2).mean((1, 2, 3))
    return (-10.0 * torch.log10(mse + 1e-8)).mean()


def rmse(dh):
    return torch.sqrt((dh * dh).sum() / dh.numel())


def median(dh):
    return torch.median(dh)


def nmad(dh):
    return 1.4826 * torch.median((dh - torch.median(dh)).abs())


def le95(dh):
    k = 1 + round(0.95 * (dh.numel() - 1))
    return torch.kthvalue(dh.abs().flatten(), k).values


def tile_scores(pred, gt, value_min, value_max, border=0.05, elev_log=True):
    """All five scores of ONE tile (1,1,H,W) on the GPU in one C-ABI call (jspsr_metrics_forward: fused crop / clamp /
    de-scale / reductions + an exact radix select for the three order statistics) -> device tensor
    (PSNR, RMSE, median, NMAD, LE95).  No host synchronisation."""
    if not pred.is_cuda or pred.shape != gt.shape or pred.numel() != pred.shape[-1] * pred.shape[-2]:
        raise ValueError("tile_scores: one (1,1,H,W) GPU tile per call")
    H, W = pred.shape[-2:]
    p, g = pred.float().contiguous(), gt.float().contiguous()
    lib = _lib.load()
    ws = torch.empty(lib.jspsr_metrics_workspace_bytes(H, W), dtype=torch.uint8, device=pred.device)
    out = torch.empty(5, dtype=torch.float32, device=pred.device)
    _lib.check(lib.jspsr_metrics_forward(p.data_ptr(), g.data_ptr(), H, W, float(border), float(value_min), float(value_max),
                                         int(bool(elev_log)), out.data_ptr(), ws.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "jspsr_metrics_forward")
    return out


SCORE_COLUMNS = ("PSNR_piq", "PSNR_local", "RMSE", "Median", "NMAD", "LE95", "Slope_local", "Slope_kornia")


COUNT_COLUMNS = ("N", "N_slope_local", "N_slope_kornia")
# SCORE_COLUMNS index -> COUNT_COLUMNS index: the count a masked column divides by (NaN where it is 0)
COUNT_OF_COLUMN = (0, 0, 0, 0, 0, 0, 1, 2)


def batch_scores(pred, gt, value_min, value_max, border=0.05, elev_log=True, valid=None):
    """All scores of a whole batch (B,1,H,W) of GPU tiles in one C-ABI call (K10, jspsr_scores_batch_forward) -> (B, 8)
    fp32 device tensor, columns ``SCORE_COLUMNS``: PSNR as piq.psnr and as the reference's local psnr (metrics.py:97-113),
    RMSE / median / NMAD / LE95 exactly as ``tile_scores`` gives them (the same elevation differences, exact selections),
    and the slope score (MeterSlope, metrics.py:595-688) in its "local" form -- RMS difference of the magnitudes of the
    unnormalised valid 3x3 Sobel pair (metrics.py:116-139) -- and its "kornia" form -- RMS of
    spatial_gradient(P) - spatial_gradient(G) (replicate pad, Sobel / 8).  The kornia form is restated from kornia's public
    source and is NOT pinned against kornia itself (not installed here); the richdem form is not built.
    One launch per call for tiles of up to 142 x 142 after the crop (one workgroup per tile, both de-scaled rasters in LDS),
    27 launches whatever B is for larger ones.  Row b does not depend on B or on the other tiles.  No host
    synchronisation.

    valid: a (B,1,H,W) bool or uint8 plane on pred's device (nonzero = valid; K20, jspsr_scores_batch_valid_forward) ->
    (scores, counts): the scores over the valid pixels of every tile, whatever pred and gt hold at the others, and the
    (B, 3) int32 device tensor ``COUNT_COLUMNS`` -- the valid pixels of the crop, the interior positions whose nine taps
    are valid (the divisor of Slope_local) and the positions whose nine replicate-clamped taps are valid (Slope_kornia).
    The ranks of the order statistics are the unmasked formulas of N.  A column whose count is 0 is NaN.  An all-ones
    plane gives the bits of the unmasked call; the launch counts are the same."""
    if not pred.is_cuda or pred.shape != gt.shape or pred.dim() != 4 or pred.shape[1] != 1:
        raise ValueError(f"batch_scores: equal (B,1,H,W) GPU tensors, got {tuple(pred.shape)} {tuple(gt.shape)}")
    B, _, H, W = pred.shape
    if valid is not None:
        if not torch.is_tensor(valid) or valid.shape != pred.shape or valid.dtype not in (torch.bool, torch.uint8) or \
                valid.device != pred.device:
            raise ValueError(f"batch_scores: valid must be a {tuple(pred.shape)} bool / uint8 plane on {pred.device}, got "
                             f"{tuple(valid.shape) if torch.is_tensor(valid) else type(valid).__name__} "
                             f"{getattr(valid, 'dtype', None)} on {getattr(valid, 'device', None)}")
    p, g = pred.float().contiguous(), gt.float().contiguous()
    lib = _lib.load()
    if valid is not None:
        v = valid.contiguous()
        v = v.view(torch.uint8) if v.dtype == torch.bool else v          # a bool is one byte, 0 or 1
        ws = torch.empty(max(lib.jspsr_scores_batch_valid_workspace_bytes(B, H, W), 16), dtype=torch.uint8, device=pred.device)
        out = torch.empty((B, len(SCORE_COLUMNS)), dtype=torch.float32, device=pred.device)
        counts = torch.empty((B, len(COUNT_COLUMNS)), dtype=torch.int32, device=pred.device)
        _lib.check(lib.jspsr_scores_batch_valid_forward(p.data_ptr(), g.data_ptr(), v.data_ptr(), B, H, W, float(border), float(value_min),
                                                        float(value_max), int(bool(elev_log)), out.data_ptr(), counts.data_ptr(),
                                                        ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "jspsr_scores_batch_valid_forward")
        return out, counts
    ws = torch.empty(max(lib.jspsr_scores_batch_workspace_bytes(B, H, W), 16), dtype=torch.uint8, device=pred.device)
    out = torch.empty((B, len(SCORE_COLUMNS)), dtype=torch.float32, device=pred.device)
    _lib.check(lib.jspsr_scores_batch_forward(p.data_ptr(), g.data_ptr(), B, H, W, float(border), float(value_min), float(value_max),
                                              int(bool(elev_log)), out.data_ptr(), ws.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "jspsr_scores_batch_forward")
    return out


def local_window():
    """The window of the reference's local ssim (evaluation/metrics.py:20-27) exactly as written there:
    exp(-(x - 5) * 2 / (2 * 1.5 * 2)), normalised in fp32.  Asymmetric and exponential, not a Gaussian; kept as is."""
    g = torch.tensor([exp(-(x - 5) * 2 / float(2 * 1.5 * 2)) for x in range(11)], dtype=torch.float32)
    return g / g.sum()


_LOCAL_WINDOW = None


def ssim(pred, gt, package="piq"):
    """Mean SSIM of prepared [0,1] tiles (B,C,H,W) on the GPU (jspsr_ssim_forward) -> 0-d device tensor.  pred is clamped
    to [0,1] (a no-op after ``prepare``).
      "piq":   piq.ssim(gt, pred, data_range=1, reduction="mean", downsample=False) (metrics.py:307-309): 11x11 Gaussian
               window (sigma 1.5), valid map, c1 = 0.01^2, c2 = 0.03^2 -- restated from piq's public source, unpinned
               against piq (not installed here); its input-range assertion (a host sync) is not reproduced.
      "local": ssim(gt, pred) of metrics.py:20-63 (:319): the window of ``local_window``, zero padding 5, H x W map."""
    global _LOCAL_WINDOW
    if package not in ("piq", "local"):
        raise NotImplementedError(f"ssim: package {package!r} (supported: 'piq', 'local')")
    if not pred.is_cuda or pred.shape != gt.shape or pred.dim() != 4:
        raise ValueError(f"ssim: expected equal (B,C,H,W) GPU tensors, got {tuple(pred.shape)} {tuple(gt.shape)}")
    same = package == "local"
    B, C, H, W = pred.shape
    if not same and (H < 11 or W < 11):
        raise ValueError(f"ssim (piq): needs H, W >= 11, got {(H, W)}")
    win = None
    if same:
        if _LOCAL_WINDOW is None:
            _LOCAL_WINDOW = (ctypes.c_float * 11)(*local_window().tolist())
        win = _LOCAL_WINDOW
    p, g = pred.float().contiguous(), gt.float().contiguous()
    lib = _lib.load()
    ws = torch.empty(lib.jspsr_ssim_workspace_bytes(B * C, H, W, int(same)), dtype=torch.uint8, device=pred.device)
    out = torch.empty(1, dtype=torch.float32, device=pred.device)
    _lib.check(lib.jspsr_ssim_forward(p.data_ptr(), g.data_ptr(), B * C, H, W, int(same), win, out.data_ptr(), ws.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "jspsr_ssim_forward")
    return out[0]


def ssim_tiles(pred, gt, package="piq", border=0.0, valid=None):
    """SSIM of every tile of a batch of UNCROPPED (B,1,H,W) GPU tiles in one call (K23, jspsr_ssim_tiles_forward: two
    launches whatever B is) -> (B,) fp32 device tensor: row b is ``ssim(*prepare(pred[b:b+1], gt[b:b+1], border),
    package)``, bit for bit; the crop is index arithmetic, nothing is copied.  No host synchronisation.

    valid: a (B,1,H,W) bool or uint8 plane on pred's device (nonzero = valid) -> (values, counts): a map element counts iff
    every pixel of its 11x11 window that lies inside the cropped tile is valid ("piq": the whole window lies inside;
    "local": taps in the zero padding are padding, not voids); values[b] is the mean of the SSIM map over tile b's counted
    elements, whatever pred and gt hold at the invalid pixels (they are read as 0 behind a select), NaN where the (B,)
    int32 device tensor `counts` is 0.  An all-ones plane gives the bits of valid=None."""
    global _LOCAL_WINDOW
    if package not in ("piq", "local"):
        raise NotImplementedError(f"ssim_tiles: package {package!r} (supported: 'piq', 'local')")
    if not pred.is_cuda or pred.shape != gt.shape or pred.dim() != 4 or pred.shape[1] != 1:
        raise ValueError(f"ssim_tiles: equal (B,1,H,W) GPU tensors, got {tuple(pred.shape)} {tuple(gt.shape)}")
    B, _, H, W = pred.shape
    if valid is not None:
        if not torch.is_tensor(valid) or valid.shape != pred.shape or valid.dtype not in (torch.bool, torch.uint8) or \
                valid.device != pred.device:
            raise ValueError(f"ssim_tiles: valid must be a {tuple(pred.shape)} bool / uint8 plane on {pred.device}, got "
                             f"{tuple(valid.shape) if torch.is_tensor(valid) else type(valid).__name__} "
                             f"{getattr(valid, 'dtype', None)} on {getattr(valid, 'device', None)}")
    same = package == "local"
    border = float(border)
    if not 0.0 <= border < 0.5:
        raise ValueError(f"ssim_tiles: border must be in [0, 0.5), got {border}")
    h, w = H - 2 * int(H * border), W - 2 * int(W * border)
    if not same and (h < 11 or w < 11):
        raise ValueError(f"ssim_tiles (piq): needs H, W >= 11 after the crop, got {(h, w)}")
    win = None
    if same:
        if _LOCAL_WINDOW is None:
            _LOCAL_WINDOW = (ctypes.c_float * 11)(*local_window().tolist())
        win = _LOCAL_WINDOW
    p, g = pred.float().contiguous(), gt.float().contiguous()
    v = None
    if valid is not None:
        v = valid.contiguous()
        v = v.view(torch.uint8) if v.dtype == torch.bool else v
    lib = _lib.load()
    ws = torch.empty(max(lib.jspsr_ssim_tiles_workspace_bytes(B, H, W, border, int(same)), 16), dtype=torch.uint8, device=pred.device)
    out = torch.empty(B, dtype=torch.float32, device=pred.device)
    counts = torch.empty(B, dtype=torch.int32, device=pred.device)
    _lib.check(lib.jspsr_ssim_tiles_forward(p.data_ptr(), g.data_ptr(), v.data_ptr() if v is not None else None, B, H, W, border,
                                            int(same), win, out.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "jspsr_ssim_tiles_forward")
    return (out, counts) if valid is not None else out


class Meter:
    """Running per-sample averages of all five scores (what PerformanceMeter.get_score reports,
    evaluation/evaluate_utils.py:26-47).  Accumulates on the device; one host sync in ``scores()``.
    GPU tiles of batch size 1 (how the reference evaluates) go through the fused HIP path (`tile_scores`); CPU tensors
    and larger batches through the same formulas as torch operators.
    ssim = "piq" | "local" adds "SSIM" (get_meter's MeterSSIM, evaluate_utils.py:75): ``ssim`` after the same
    ``prepare`` (border crop, clamp), on the GPU only.  With ssim = None (the default) the five scores are unchanged."""

    NAMES = ("PSNR", "RMSE", "Median", "NMAD", "LE95")

    def __init__(self, value_min, value_max, border=0.05, elev_log=True, ssim=None):
        if ssim not in (None, "piq", "local"):
            raise NotImplementedError(f"Meter: ssim package {ssim!r} (supported: None, 'piq', 'local')")
        self.vmin, self.vmax, self.border, self.elev_log = value_min, value_max, border, elev_log
        self.ssim = ssim
        self.names = self.NAMES + (("SSIM",) if ssim else ())
        self.sums, self.n = None, 0

    def _with_ssim(self, vals, pred, gt):
        if not self.ssim:
            return vals
        p, g = prepare(pred.float(), gt.float(), self.border)
        return torch.cat((vals, ssim(p, g, self.ssim).view(1)))

    @torch.no_grad()
    def update(self, pred, gt):
        if pred.is_cuda and pred.dim() == 4 and pred.shape[0] == 1 and pred.shape[1] == 1:
            vals = self._with_ssim(tile_scores(pred, gt, self.vmin, self.vmax, self.border, self.elev_log), pred, gt)
            self.sums = vals if self.sums is None else self.sums + vals
            self.n += 1
            return
        p, g = prepare(pred.float(), gt.float(), self.border)
        dh = descale_data(p, self.vmin, self.vmax, self.elev_log) - descale_data(g, self.vmin, self.vmax, self.elev_log)
        vals = self._with_ssim(torch.stack((psnr(p, g), rmse(dh), median(dh), nmad(dh), le95(dh))), pred, gt)
        self.sums = vals if self.sums is None else self.sums + vals
        self.n += 1

    def scores(self):
        v = (self.sums / max(self.n, 1)).tolist()
        return dict(zip(self.names, v))
