"""fp64 numpy restatement of the masked per-tile scores (K20: jspsr_scores_batch_valid_forward, `metrics.batch_scores(valid=)`),
built on the functions of tests/eval_ref.py.  CPU only.

The reference's meters have no mask, so nothing here can be generated from it; the pin is by construction and
tests/test_masked_eval_cpu.py checks it: with an all-ones plane `tile_scores` below IS `eval_ref.tile_scores`, and with a
rectangular valid region it is `eval_ref.tile_scores` of the cropped tile.

One (H, W) tile, `valid` an (H, W) plane (nonzero = valid), cropped by the same int(H * border) / int(W * border):
  * N = the valid pixels of the crop; the valid differences are COMPACTED (row-major order) and columns 0-5 are
    eval_ref's expressions over them, the ranks K10's formulas of N: lower median (N - 1) // 2, LE95 1 + round(0.95 (N - 1));
  * column 6: the Sobel magnitudes of eval_ref.sobel_local at the N_sl interior positions whose nine taps are all valid,
    divisor N_sl;
  * column 7: eval_ref.spatial_gradient (replicate pad) at the N_sk positions whose nine replicate-clamped taps are all
    valid (K19's rule for the Grad loss, tests/masked_loss_ref.py: counted), divisor 2 N_sk;
  * a column whose count is 0 is NaN.
pred and gt at the masked pixels are replaced by 0 first: they have no influence by definition (a counted Sobel output
reads valid taps only), and NaN / inf there would only raise numpy warnings."""
from __future__ import annotations

import math

import numpy as np

from tests import eval_ref as E


def crop_plane(valid, border):
    v = np.asarray(valid) != 0
    H, W = v.shape[-2:]
    bh, bw = int(H * border), int(W * border)
    return v[..., bh:H - bh, bw:W - bw]


def min3(v):
    """(h, w) bool -> (h - 2, w - 2) bool: all nine taps of the valid 3x3 window set."""
    out = np.ones((v.shape[0] - 2, v.shape[1] - 2), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out &= v[dy:dy + out.shape[0], dx:dx + out.shape[1]]
    return out


def counted_local(v):
    """(h - 2, w - 2): the interior positions whose nine taps are valid."""
    return min3(v)


def counted_kornia(v):
    """(h, w): the positions whose nine replicate-clamped taps are valid."""
    return min3(np.pad(v, 1, mode="edge"))


def counts(valid, border):
    v = crop_plane(valid, border)
    return np.array([int(v.sum()), int(counted_local(v).sum()), int(counted_kornia(v).sum())], dtype=np.int64)


def tile_scores(pred, gt, valid, vmin, vmax, border, elev_log, elev_dtype=np.float32):
    """-> ((8,) fp64 scores, (3,) int64 counts {N, N_sl, N_sk}) of ONE (H, W) tile."""
    v = crop_plane(valid, border)
    p, g = E.prepare(np.where(np.asarray(valid) != 0, pred, 0.0), np.where(np.asarray(valid) != 0, gt, 0.0), border)
    c_sl, c_sk = counted_local(v), counted_kornia(v)
    n, n_sl, n_sk = int(v.sum()), int(c_sl.sum()), int(c_sk.sum())
    out = np.full(8, np.nan)
    P, G = E.descale(p, vmin, vmax, elev_log, elev_dtype), E.descale(g, vmin, vmax, elev_log, elev_dtype)
    if n:
        mse = float(np.mean(((p - g) ** 2)[v]))
        dh = (P.astype(elev_dtype) - G.astype(elev_dtype)).astype(np.float64)[v]
        s = np.sort(dh)
        med = s[(n - 1) // 2]
        dev = np.sort(np.abs(dh - med))
        k95 = 1 + round(0.95 * (n - 1))
        out[:6] = (-10.0 * math.log10(mse + 1e-8),
                   100.0 if mse == 0 else 20.0 * math.log10(1.0 / math.sqrt(mse)),
                   math.sqrt(float(np.sum(dh * dh)) / n),
                   med,
                   1.4826 * dev[(n - 1) // 2],
                   np.sort(np.abs(dh))[k95 - 1])
    if n_sl:
        out[6] = math.sqrt(float(np.mean(((E.sobel_local(P) - E.sobel_local(G)) ** 2)[c_sl])))
    if n_sk:
        out[7] = math.sqrt(float(np.mean(((E.spatial_gradient(P) - E.spatial_gradient(G)) ** 2)[:, c_sk])))
    return out, np.array([n, n_sl, n_sk], dtype=np.int64)


def batch_scores(pred, gt, valid, vmin, vmax, border, elev_log, elev_dtype=np.float32):
    """(N,1,H,W) x 3 -> ((N, 8) fp64, (N, 3) int64)."""
    rows = [tile_scores(pred[i, 0], gt[i, 0], valid[i, 0], vmin, vmax, border, elev_log, elev_dtype) for i in range(pred.shape[0])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
