"""numpy restatement of the whole-set validation summary, the yardstick of tests/test_summary_cpu.py and
tests/test_summary_gpu.py.

The reference's `summarise_evaluation` (utils/utils.py:970-1368) cannot be imported where the tests run: rasterio,
geopandas, rioxarray and natsort are absent.  This file restates its lines :1238-1356 one by one on float32 arrays that
are already in memory (the reference reads them from GeoTIFF files):
  :1276-1306  every raster loses int(patch_size * val_border) pixels per side; a prediction that already has the cropped
              size (the merged mosaic) is taken whole                                          -> `crop`
  :1323-1335  error = raster - gt in float32, the scenes' errors concatenated                  -> `errors`
  :1337-1356  np.median, sqrt(mean(e^2)), 1.4826 median|e - median|, np.percentile(|e|, 95), 20 log10(max / rmse) -> `scores`
`scores` takes the mean of the squares and the percentile in float64 (the definition the package documents; the
reference's own float32 forms depend on numpy's summation order and, for the percentile, on the numpy version), and
gives the six bracketing order statistics from `np.sort` at the ranks `ranks` names.
The scene assembly (save_prediction_to_disk, evaluation/evaluate_utils.py:242-271, then merge_dem, utils/utils.py:914-967
called at :1272) is restated as the composition of the package's own steps: clamp -> descale_data -> + base -> merge_tiles.
"""
import math

import numpy as np
import torch

from jspsr_amd import metrics as M
from jspsr_amd import tiles as T

COLUMNS = ("RMSE", "Median", "NMAD", "LE95", "PSNR")


def ranks(n):
    """0-based (median lo, median hi, LE95 lo, LE95 hi): np.median's two middle elements, np.percentile's neighbours."""
    v = 0.95 * (n - 1)
    lo = int(math.floor(v))
    return (n - 1) // 2, n // 2, lo, min(lo + 1, n - 1)


def crop(a, b, gt_shape):
    """utils.py:1276-1306 for one raster: b = int(patch_size * val_border)."""
    a = np.asarray(a, dtype=np.float32)
    h1, w1 = gt_shape
    if b > 0 and a.shape == (h1, w1):
        a = a[b:h1 - b, b:w1 - b]
    return a.flatten()


def errors(rasters, gts, b):
    """utils.py:1247-1335: the concatenated float32 errors of all scenes."""
    out = np.array([]).astype(np.float32)
    for r, g in zip(rasters, gts):
        g = np.asarray(g, dtype=np.float32)
        arr_gt = crop(g, b, g.shape)
        arr = crop(r, b, g.shape)
        assert arr.shape == arr_gt.shape, f"{arr.shape} {arr_gt.shape}"
        out = np.concatenate((out, arr - arr_gt))
    return out


def scores(e, value_max):
    """utils.py:1337-1356 on one float32 error vector -> dict: the five scores (Median as numpy gives it, a float32; the
    others as Python floats from float64 arithmetic) and "brackets", the six order statistics
    (median lo, hi, MAD lo, hi, LE95 lo, hi)."""
    e = np.asarray(e)
    assert e.dtype == np.float32 and e.ndim == 1
    m0, m1, l0, l1 = ranks(e.size)
    with np.errstate(all="ignore"):
        median = np.median(e)
        rmse = math.sqrt(np.mean(e.astype(np.float64) ** 2))
        dev = np.abs(e - median)
        nmad = 1.4826 * float(np.median(dev))
        le95 = float(np.percentile(np.abs(e).astype(np.float64), 95))
        psnr = float(20 * np.log10(np.float64(value_max) / np.float64(rmse)))
    s, d, a = np.sort(e), np.sort(dev), np.sort(np.abs(e))
    return {"RMSE": rmse, "Median": median, "NMAD": nmad, "LE95": le95, "PSNR": psnr,
            "brackets": np.array([s[m0], s[m1], d[m0], d[m1], a[l0], a[l1]], dtype=np.float32)}


def summarise(gts, candidates, b, value_max):
    """candidates {name: list of rasters} -> (offline {name: scores}, online {name: means of the per-scene scores},
    per_scene {name: [scores per scene]})."""
    offline, online, per_scene = {}, {}, {}
    for name, rasters in candidates.items():
        offline[name] = scores(errors(rasters, gts, b), value_max)
        per_scene[name] = [scores(errors([r], [g], b), value_max) for r, g in zip(rasters, gts)]
        online[name] = {k: sum(float(s[k]) for s in per_scene[name]) / len(gts) for k in COLUMNS}
    return offline, online, per_scene


def assemble(tiles, base, full, border, elev_min, elev_max, elev_log):
    """One scene's metre raster from its (n, 1, k, k) tile predictions, on the tiles' device: elementwise clamp ->
    metrics.descale_data -> + base -> tiles.merge_tiles; a single tile that is the whole scene stays uncropped."""
    m = M.descale_data(torch.clamp(tiles.float(), 0.0, 1.0), elev_min, elev_max, elev_log)
    m = m + torch.tensor(np.float32(base), dtype=torch.float32, device=tiles.device)
    if tiles.shape[0] == 1:
        return m[0, 0]
    return T.merge_tiles(m, full, border)


def ulps(got, want):
    """|got - want| in units of the fp32 spacing at want (want: the float64 value; got: the fp32 result)."""
    got, want = np.float64(got), np.float64(want)
    if np.isinf(want) or np.isnan(want):
        return 0.0 if (got == want or (np.isnan(got) and np.isnan(want))) else np.inf
    return abs(got - want) / np.float64(np.spacing(np.float32(abs(want))))


def check_row(row, ref, tag=""):
    """One (11,) output row against `scores`: brackets equal as values, Median bit-equal, NMAD / LE95 / PSNR within 1 fp32
    ulp of the float64 value, RMSE within 2 (the order of the sum).  Prints each figure before asserting."""
    row = np.asarray(row, dtype=np.float32)
    u = {k: ulps(row[j], ref[k]) for j, k in enumerate(COLUMNS) if k != "Median"}
    print(tag, "ulps", {k: round(float(v), 3) for k, v in u.items()}, "median", row[1], ref["Median"])
    assert np.array_equal(row[5:11], ref["brackets"]), (tag, row[5:11], ref["brackets"])
    assert np.float32(row[1]).tobytes() == np.float32(ref["Median"]).tobytes(), (tag, row[1], ref["Median"])
    for k in ("NMAD", "LE95", "PSNR"):
        assert u[k] <= 1.0, (tag, k, row[COLUMNS.index(k)], ref[k], u[k])
    assert u["RMSE"] <= 2.0, (tag, row[0], ref["RMSE"], u["RMSE"])
