"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/g12_eval.npz: the validation pass's numbers made by the reference's
own code (evaluation.metrics MeterPSNR("local"), MeterRMSE, MeterMedian, MeterNMAD, MeterLE95, MeterSlope("local"),
MeterSSIM("local"); evaluation.evaluate_utils validate_results, do_eval), imported as tools/gen_golden_losses.py does:
placeholder modules for the packages this image lacks.  `MeterSlope.__init__` moves its Sobel module to a GPU;
`torch.nn.Module.cuda` returns the module itself for this run, so the meters score CPU tensors.
MeterPSNR("piq"), MeterSSIM("piq") and MeterSlope("kornia" | "richdem") need packages that are not installed and are
NOT generated (tests/eval_ref.py restates the first and the kornia slope; see its docstring).

Run where the reference tree is available (never on the GPU box):

    python tools/gen_golden_eval.py

Inputs come from numpy's legacy RandomState stream (tests/eval_ref.py:tiles); the fixture stores the seed and checksums,
so the tests regenerate them and fail on a mismatch.  The reference evaluates one tile per update: each meter's running
total is read after every update and differenced, which gives its per-sample values.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402
from tests import eval_ref as E  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g12_eval.npz")
TOTALS = {"PSNR_local": "total_psnr", "RMSE": "total_rmse", "Median": "total_median", "NMAD": "total_nmad",
          "LE95": "total_le95", "Slope_local": "total_rmse", "SSIM_local": "total_ssim"}


class _Placeholder(types.ModuleType):
    """A module whose every attribute exists and does nothing: enough for `import x` / `from x import y`."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f))


def placeholders(names):
    for name in names:
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Placeholder(name)
            if "." in name:
                parent, child = name.rsplit(".", 1)
                setattr(sys.modules[parent], child, sys.modules[name])


def total_attr(meter, name):
    attr = TOTALS[name]
    if not hasattr(meter, attr):      # the order-statistic meters name their totals after themselves
        attr = [a for a in vars(meter) if a.startswith("total_") and a != "total_n"][0]
    return attr


def main():
    G.import_reference()
    placeholders(["piq", "skimage", "skimage.metrics", "kornia", "kornia.filters", "richdem", "hide_warnings", "affine",
                  "natsort", "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.axes_grid1", "seaborn", "pandas",
                  "prettytable", "rasterio", "rasterio.features", "rioxarray", "rioxarray.merge", "geopandas", "mapply",
                  "torchinfo"])
    torch.nn.Module.cuda = lambda self, device=None: self       # MeterSlope.__init__: Sobel().cuda()
    import evaluation.metrics as em
    import evaluation.evaluate_utils as eu

    store = {"seed": np.int64(E.SEED), "vmin": np.float64(E.VMIN), "vmax": np.float64(E.VMAX)}
    for name in E.SETS:
        pred, gt = E.tiles(name)
        store[f"{name}_checksum"] = np.float64(E.checksum([pred, gt]))
        tp, tg = torch.from_numpy(pred), torch.from_numpy(gt)
        n = pred.shape[0]
        for border in E.BORDERS:
            for lg in (True, False):
                key = E.case_key(name, border, lg)
                kw = dict(border=border, value_min=E.VMIN, value_max=E.VMAX, verbose=False)
                meters = {"PSNR_local": em.MeterPSNR("local", psnr_type="rgb", **kw), "RMSE": em.MeterRMSE("local", **kw),
                          "Median": em.MeterMedian("local", **kw), "NMAD": em.MeterNMAD("local", **kw),
                          "LE95": em.MeterLE95("local", **kw), "Slope_local": em.MeterSlope("local", **kw),
                          "SSIM_local": em.MeterSSIM("local", **kw)}
                per = {m: [] for m in meters}
                rmse64 = em.MeterRMSE("local", **kw)
                for i in range(n):
                    meta = [{"subset": "val_set", "id": f"g12-{name}-{i:03d}-0"}]
                    for m, meter in meters.items():
                        attr = total_attr(meter, m)
                        before = getattr(meter, attr)
                        meter.update(tp[i:i + 1], tg[i:i + 1], meta=meta, elev_log=lg)
                        per[m].append(getattr(meter, attr) - before)
                    rmse64.update(tp[i:i + 1].double(), tg[i:i + 1].double(), meta=meta, elev_log=lg)
                store[f"{key}_sample_rmse"] = np.array(meters["RMSE"].sample_rmse, dtype=np.float64)
                store[f"{key}_sample_rmse64"] = np.array(rmse64.sample_rmse, dtype=np.float64)
                ids = list(meters["RMSE"].sample_id)
                # the restatement must agree with the reference before anything is stored (bounds: tests/test_eval_cpu.py)
                ref = E.batch_scores(pred, gt, E.VMIN, E.VMAX, border, lg)
                col = {c: ref[:, j] for j, c in enumerate(E.COLUMNS)}
                ref64 = E.batch_scores(pred, gt, E.VMIN, E.VMAX, border, lg, elev_dtype=np.float64)
                assert np.abs(ref64[:, 2] - store[f"{key}_sample_rmse64"]).max() <= 1e-9 * ref64[:, 2].min(), key
                for m in ("RMSE", "Slope_local"):
                    assert np.all(np.abs(col[m] - np.array(per[m])) <= 2e-3 + 1e-5 * np.abs(per[m])), (key, m)
                assert np.abs(col["PSNR_local"] - np.array(per["PSNR_local"])).max() <= 1e-3, key
                for m in ("Median", "NMAD", "LE95"):
                    tol = 2.5e-4 + 1e-6 * np.abs(per[m]) if lg else 1e-6 * np.abs(per[m]) + 1e-12
                    assert np.all(np.abs(col[m] - np.array(per[m])) <= tol), (key, m, col[m], per[m])
                for m, meter in meters.items():
                    store[f"{key}_{m}"] = np.array(per[m], dtype=np.float64)
                # averages and the worst three (get_score pops from sample_rmse: taken last)
                worst = E.worst(meters["RMSE"].sample_rmse)
                for m, meter in meters.items():
                    if m != "RMSE":
                        store[f"{key}_avg_{m}"] = np.float64(meter.get_score())
                rm = meters["RMSE"]
                store[f"{key}_avg_RMSE"] = np.float64(rm.get_score())
                gone = [i for i in ids if i not in rm.sample_id]          # what get_score removed, in id order
                assert sorted(ids[j] for j, _ in worst) == sorted(gone), (key, worst, gone)
                store[f"{key}_worst_index"] = np.array([j for j, _ in worst], dtype=np.int64)
                store[f"{key}_worst_value"] = np.array([v for _, v in worst], dtype=np.float64)
    # --- the two pure functions: recorded argument / result rows ---
    rs = np.random.RandomState(E.SEED + 9)
    rows = []
    names = ["PSNR", "RMSE", "SSIM", "Median", "NMAD", "LE95"]
    for t in range(40):
        keys = [k for k in names if rs.random_sample() < 0.6] or ["RMSE"]
        cur = {k: float(np.round(rs.uniform(0.0, 40.0), 3)) for k in keys}
        ref = {k: float(np.round(rs.uniform(0.0, 40.0), 3)) for k in keys}
        if t % 5 == 0:
            ref[keys[0]] = 0.0                                         # the "reference is 0" escape
        if t % 7 == 0:
            ref[keys[-1]] = cur[keys[-1]]                              # a tie
        best = [None, "RMSE", ["RMSE"], ["PSNR", "SSIM"], "Slope", [], ["RMSE", "PSNR"], "psnr"][t % 8]
        row = {"current": cur, "reference": ref, "best_metric": best}
        try:
            better, kept = eu.validate_results(dict(cur), dict(ref), best)
            row.update(better=bool(better), kept=kept, raises=None)
        except KeyError:        # a best_metric list of which only some names are scored: the reference indexes the missing one
            row.update(better=None, kept=None, raises="KeyError")
        rows.append(row)
    store["validate_rows"] = np.array(json.dumps(rows))
    args, res = [], []
    for epochs, start, warm, interval, vstart in ((20, 0, 2, 1, 1), (30, 0, 3, 5, 10), (25, 4, 2, None, 1), (12, 0, 0, 4, 6),
                                                  (50, 10, 5, 7, 20)):
        for cur in range(start, epochs):
            args.append([epochs, cur, start, warm, -1 if interval is None else interval, vstart])
            res.append(bool(eu.do_eval(epochs, cur, start, warm, interval, vstart)))
    store["do_eval_args"] = np.array(args, dtype=np.int64)
    store["do_eval_result"] = np.array(res, dtype=np.bool_)
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
