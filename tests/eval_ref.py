"""fp64 numpy restatement of the eight columns of `jspsr_amd.metrics.batch_scores` (K10, csrc/scores.hip) and the seeded
inputs of tests/golden/g12_eval.npz (tools/gen_golden_eval.py).  CPU only; the tests compare the kernels and
`evaluate.PerformanceMeter` against these and against the reference-made numbers of the fixture.

Restates evaluation/metrics.py: MeterBase._prepare :147-199, psnr :97-113, Sobel :116-139, MeterPSNR :229-250, MeterRMSE
:372-384, MeterMedian :453, MeterNMAD :508-510, MeterLE95 :565-568, MeterSlope :648-673, and ToDEM.descale_data
(data/data_utils.py:441-457).  The inputs are fp32 (what the network and the loader produce).  The de-scaled rasters are
fp32 tensors in the reference and in the kernel, and that rounding (half an ulp of a ~500 m elevation, 3e-5 m) is as
large as the order statistics of a good prediction's differences are small; so by default the de-scaling is done in fp32
here too (`elev_dtype`), with the reference's two roundings (multiply, then add), and everything after it -- the
differences' sums, the selections, the Sobel terms, the square roots -- in fp64, where the reference's meters stay in
fp32.  `elev_dtype=np.float64` gives the all-fp64 value (held to the reference's RMSE meter run on fp64 tensors).

Column 7 (MeterSlope "kornia") is restated from kornia's public source -- spatial_gradient(mode="sobel", order=1,
normalized=True): replicate padding, the 3x3 Sobel pair divided by 8, both components kept -- and is UNPINNED against
kornia itself, which is not installed here.  The closest pin is csrc/train_step.hip's Grad term, which restates the same
operator and is held to the reference-made loss numbers."""
from __future__ import annotations

import math

import numpy as np

SEED = 2612
VMIN, VMAX = -80.0, 929.0
SETS = {"sq": (8, 128, 128), "rect": (4, 96, 160)}        # name -> (tiles, H, W)
BORDERS = (0.05, 0.0)
COLUMNS = ("PSNR_piq", "PSNR_local", "RMSE", "Median", "NMAD", "LE95", "Slope_local", "Slope_kornia")


def tiles(name):
    """(pred, gt) fp32 (N,1,H,W) in the network's range from numpy's legacy RandomState stream: smooth DEM-like fields
    plus noise that grows with the sample index (distinct RMSE per sample), one prediction pixel above 1 and one below 0
    inside every crop, a patch where pred == gt (zeros of dh, ties)."""
    n, H, W = SETS[name]
    rs = np.random.RandomState(SEED + (0 if name == "sq" else 1))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64) / max(H, W)
    gt = np.empty((n, 1, H, W))
    pred = np.empty((n, 1, H, W))
    for i in range(n):
        a, f, ph = rs.uniform(0.45, 0.6), rs.uniform(2.0, 7.0), rs.uniform(0.0, 2 * math.pi)
        gt[i, 0] = a + 0.15 * np.sin(f * xx + ph) * np.cos(0.8 * f * yy + ph) + 0.08 * yy + rs.normal(0.0, 0.002, (H, W))
        pred[i, 0] = gt[i, 0] + rs.normal(0.0003 * ((i * 5) % 7 - 2), 0.0015 * (1 + (i * 3) % 5), (H, W))
    pred[..., 20:26, 30:41] = gt[..., 20:26, 30:41]
    pred[..., H // 2, W // 3] = 1.3
    pred[..., H // 3, W // 2] = -0.2
    return pred.astype(np.float32), gt.astype(np.float32)


def checksum(arrays):
    return float(sum(np.asarray(a, dtype=np.float64).sum() * (i + 1) + np.abs(np.asarray(a, dtype=np.float64)).sum()
                     for i, a in enumerate(arrays)))


def prepare(pred, gt, border):
    """(..., H, W) fp32 -> cropped fp64 pair, the prediction clamped to [0, 1]."""
    H, W = pred.shape[-2:]
    bh, bw = int(H * border), int(W * border)
    p = np.asarray(pred, dtype=np.float64)[..., bh:H - bh, bw:W - bw]
    g = np.asarray(gt, dtype=np.float64)[..., bh:H - bh, bw:W - bw]
    return np.clip(p, 0.0, 1.0), g


def descale(v, vmin, vmax, elev_log, elev_dtype=np.float32):
    """ToDEM.descale_data in `elev_dtype` arithmetic (one rounding per operation, as torch's tensor expressions),
    returned as fp64."""
    t = elev_dtype
    v = np.asarray(v).astype(t)
    if elev_log:
        out = np.exp(v * t(math.log(vmax - vmin))) + t(vmin)
    else:
        out = v * t(vmax - vmin) + t(vmin)
    return out.astype(np.float64)


def sobel_local(z):
    """Sobel.forward (metrics.py:116-139) of one (h, w) raster: valid cross-correlation, magnitude."""
    a, b, c = z[:-2, :-2], z[:-2, 1:-1], z[:-2, 2:]
    e, f = z[1:-1, :-2], z[1:-1, 2:]
    g, h, k = z[2:, :-2], z[2:, 1:-1], z[2:, 2:]
    gx = 2 * a - 2 * c + 4 * e - 4 * f + 2 * g - 2 * k
    gy = 2 * a + 4 * b + 2 * c - 2 * g - 4 * h - 2 * k
    return np.sqrt(gx * gx + gy * gy)


def spatial_gradient(z):
    """kornia.filters.spatial_gradient(mode='sobel', order=1, normalized=True) of one (h, w) raster -> (2, h, w)."""
    q = np.pad(z, 1, mode="edge")
    a, b, c = q[:-2, :-2], q[:-2, 1:-1], q[:-2, 2:]
    e, f = q[1:-1, :-2], q[1:-1, 2:]
    g, h, k = q[2:, :-2], q[2:, 1:-1], q[2:, 2:]
    gx = ((c - a) + 2 * (f - e) + (k - g)) / 8.0
    gy = ((g - a) + 2 * (h - b) + (k - c)) / 8.0
    return np.stack((gx, gy))


def tile_scores(pred, gt, vmin, vmax, border, elev_log, elev_dtype=np.float32):
    """The eight columns of ONE (H, W) tile, fp64 (see the module docstring for `elev_dtype`)."""
    p, g = prepare(pred, gt, border)
    mse = float(np.mean((p - g) ** 2))
    P, G = descale(p, vmin, vmax, elev_log, elev_dtype), descale(g, vmin, vmax, elev_log, elev_dtype)
    dh = (P.astype(elev_dtype) - G.astype(elev_dtype)).astype(np.float64).ravel()
    n = dh.size
    s = np.sort(dh)
    med = s[(n - 1) // 2]                                         # torch.median: the lower middle element
    dev = np.sort(np.abs(dh - med))
    k95 = 1 + round(0.95 * (n - 1))                               # kthvalue's 1-based k
    gp, gg = spatial_gradient(P), spatial_gradient(G)
    return np.array([
        -10.0 * math.log10(mse + 1e-8),
        100.0 if mse == 0 else 20.0 * math.log10(1.0 / math.sqrt(mse)),
        math.sqrt(float(np.sum(dh * dh)) / n),
        med,
        1.4826 * dev[(n - 1) // 2],
        np.sort(np.abs(dh))[k95 - 1],
        math.sqrt(float(np.mean((sobel_local(P) - sobel_local(G)) ** 2))),
        math.sqrt(float(np.mean((gp - gg) ** 2))),
    ])


def batch_scores(pred, gt, vmin, vmax, border, elev_log, elev_dtype=np.float32):
    """(N,1,H,W) -> (N, 8) fp64."""
    return np.stack([tile_scores(pred[i, 0], gt[i, 0], vmin, vmax, border, elev_log, elev_dtype) for i in range(pred.shape[0])])


def worst(values, n=3):
    """MeterRMSE.get_score's worst-n walk (metrics.py:404-420): argmax, pop, repeat -> [(index, value)]; empty unless
    more than 3 samples."""
    vals = list(values)
    idx = list(range(len(vals)))
    out = []
    if len(vals) > 3:
        for _ in range(n):
            j = int(np.argmax(vals))
            out.append((idx[j], vals[j]))
            vals.pop(j)
            idx.pop(j)
    return out


def case_key(name, border, elev_log):
    return f"{name}_b{int(round(border * 100))}_{'log' if elev_log else 'lin'}"
