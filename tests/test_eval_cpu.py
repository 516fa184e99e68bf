"""The validation pass without a GPU: tests/eval_ref.py and `evaluate.PerformanceMeter` (CPU tensors) against the numbers
the reference's own meters produced (tests/golden/g12_eval.npz, tools/gen_golden_eval.py), and the two pure functions
against their recorded rows.

Bounds.  The reference's meters compute in fp32 (`psnr` casts to float32, `Sobel` holds fp32 weights, the de-scaled rasters
are fp32 tensors); against reference-made meter numbers the project uses 2e-3 + 1e-5 |ref| for RMSE and the slope, 1e-3 dB
for PSNR, 2.5e-4 m for the order statistics under log scaling (torch's and numpy's fp32 exp differ by an ulp of a ~900 m
elevation) and 1e-6 relative under linear scaling (tests/test_host_side_golden.py:84-87, :199-201).  The last one can hold
only because tests/eval_ref.py rounds the de-scaled rasters to fp32 as the reference does (its docstring); with all-fp64
elevations the order statistics of these tiles sit up to 4e-5 m from the reference's.  The reference's RMSE meter also
runs on fp64 tensors: the all-fp64 restatement is held to that run at 1e-9 relative."""
import json
import os

import numpy as np
import pytest
import torch

from jspsr_amd import evaluate as EV
from tests import eval_ref as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_eval.npz")
CASES = [(name, border, lg) for name in E.SETS for border in E.BORDERS for lg in (True, False)]
REF_COLUMNS = {"PSNR_local": 1, "RMSE": 2, "Median": 3, "NMAD": 4, "LE95": 5, "Slope_local": 6}
CONFIG = {"PSNR": {"package": "local"}, "RMSE": {"package": "local"}, "Median": {"package": "local"},
          "NMAD": {"package": "local"}, "LE95": {"package": "local"}, "Slope": {"package": "local"},
          "SSIM": {"package": "local"}}
FIXTURE_NAME = {"PSNR": "PSNR_local", "RMSE": "RMSE", "Median": "Median", "NMAD": "NMAD", "LE95": "LE95",
                "Slope": "Slope_local", "SSIM": "SSIM_local"}


@pytest.fixture(scope="module")
def g12():
    return dict(np.load(GOLDEN))


def bound(metric, ref, elev_log):
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    if metric in ("RMSE", "Slope_local", "Slope"):
        return 2e-3 + 1e-5 * ref
    if metric in ("PSNR_local", "PSNR"):
        return 1e-3 + 0 * ref
    if metric in ("SSIM_local", "SSIM"):
        return 1e-5 + 0 * ref         # fp32 sums of an H x W map of values near 1 (no reference bound in the project: 100 ulp)
    return 2.5e-4 + 1e-6 * ref if elev_log else 1e-6 * ref + 1e-12


def test_fixture_inputs_regenerate(g12):
    assert int(g12["seed"]) == E.SEED and float(g12["vmin"]) == E.VMIN and float(g12["vmax"]) == E.VMAX
    for name, (n, H, W) in E.SETS.items():
        pred, gt = E.tiles(name)
        assert pred.shape == gt.shape == (n, 1, H, W) and pred.dtype == np.float32
        assert E.checksum([pred, gt]) == float(g12[f"{name}_checksum"]), name
        assert pred.max() > 1.0 and pred.min() < 0.0
    assert E.SETS["sq"][0] >= 8 and E.SETS["rect"][0] >= 4


@pytest.mark.parametrize("name,border,lg", CASES)
def test_restatement_matches_reference_meters(g12, name, border, lg):
    key = E.case_key(name, border, lg)
    pred, gt = E.tiles(name)
    got = E.batch_scores(pred, gt, E.VMIN, E.VMAX, border, lg)
    for metric, col in REF_COLUMNS.items():
        ref = g12[f"{key}_{metric}"]
        err = np.abs(got[:, col] - ref)
        print(key, metric, "max err", err.max(), "bound", bound(metric, ref, lg).min())
        assert np.all(err <= bound(metric, ref, lg)), (key, metric, got[:, col], ref)
        avg = float(g12[f"{key}_avg_{metric}"])
        assert abs(got[:, col].mean() - avg) <= float(bound(metric, avg, lg)), (key, metric)
    assert np.array_equal(g12[f"{key}_sample_rmse"], g12[f"{key}_RMSE"])      # the record and the differenced totals agree
    got64 = E.batch_scores(pred, gt, E.VMIN, E.VMAX, border, lg, elev_dtype=np.float64)
    r64 = g12[f"{key}_sample_rmse64"]
    assert np.all(np.abs(got64[:, 2] - r64) <= 1e-9 * r64), (key, got64[:, 2], r64)
    worst = E.worst(got[:, 2])
    assert [j for j, _ in worst] == list(g12[f"{key}_worst_index"])


@pytest.mark.parametrize("name,border,lg", CASES)
def test_performance_meter_cpu_matches_reference(g12, name, border, lg):
    key = E.case_key(name, border, lg)
    pred, gt = (torch.from_numpy(a) for a in E.tiles(name))
    n = pred.shape[0]
    tables = []
    for bs in (1, 3, n):
        meter = EV.PerformanceMeter(CONFIG, E.VMIN, E.VMAX, border=border, elev_log=lg)
        for lo in range(0, n, bs):
            meter.update(pred[lo:lo + bs], gt[lo:lo + bs], meta=[{"id": f"tile{i}"} for i in range(lo, min(lo + bs, n))])
        scores = meter.get_score()
        assert list(scores) == list(CONFIG)
        for k, v in scores.items():
            ref = float(g12[f"{key}_avg_{FIXTURE_NAME[k]}"])
            tol = 2e-3 + 1e-5 * abs(ref)
            print(key, bs, k, v, ref)
            assert abs(v - ref) <= tol, (key, bs, k, v, ref)
        worst = meter.worst("RMSE", n=3)
        assert [i for i, _ in worst] == [f"tile{j}" for j in g12[f"{key}_worst_index"]]
        assert np.allclose([v for _, v in worst], g12[f"{key}_worst_value"], rtol=1e-5, atol=2e-3)
        t, meta = meter.table()
        assert t.shape == (n, len(CONFIG)) and len(meta) == n and len(meter) == n
        # per sample, every metric, within the per-metric bounds of the reference-made numbers
        for j, k in enumerate(CONFIG):
            ref = g12[f"{key}_{FIXTURE_NAME[k]}"]
            assert np.all(np.abs(t[:, j] - ref) <= bound(k, ref, lg)), (key, bs, k, t[:, j], ref)
        tables.append(t)
    assert np.array_equal(tables[0], tables[1]) and np.array_equal(tables[0], tables[2])


def test_performance_meter_bookkeeping():
    pred, gt = (torch.from_numpy(a[:3]) for a in E.tiles("rect"))
    meter = EV.PerformanceMeter({"rmse": {"package": "local"}, "psnr": {"package": "PIQ"}, "SLOPE": {"package": "kornia"}},
                                E.VMIN, E.VMAX, border=0.0, elev_log=False)
    meter.update(pred, gt)
    assert meter.worst("RMSE") == []                        # three samples: not more than 3
    ref = E.batch_scores(pred.numpy(), gt.numpy(), E.VMIN, E.VMAX, 0.0, False)
    s = meter.get_score()
    assert list(s) == ["rmse", "psnr", "SLOPE"]
    assert abs(s["rmse"] - ref[:, 2].mean()) < 2e-3 and abs(s["psnr"] - ref[:, 0].mean()) < 1e-3
    assert abs(s["SLOPE"] - ref[:, 7].mean()) < 2e-3 + 1e-5 * ref[:, 7].mean()
    meter.update(pred[:1], gt[:1])
    w = meter.worst("rmse", n=2)                            # no meta: the sample's index; a tie keeps the first occurrence
    t, _ = meter.table()
    assert len(w) == 2 and w[0][0] == int(np.argmax(t[:, 0])) and t[0, 0] == t[3, 0]
    meter.reset()
    assert len(meter) == 0
    with pytest.raises(ValueError):
        meter.get_score()
    with pytest.raises(ValueError):
        meter.update(pred[:, 0], gt[:, 0])
    with pytest.raises(ValueError):
        meter.update(pred, gt, meta=[{}])


@pytest.mark.parametrize("config", [{"PSNR": {"package": "skimage"}}, {"Slope": {"package": "richdem"}},
                                    {"SSIM": {"package": "skimage"}}, {"RMSE": {"package": "piq"}}, {"MAE": {"package": "local"}},
                                    {"RMSE": {"package": "local"}, "Slope": {}, "Foo": None}])
def test_unknown_metric_or_package_raises(config):
    with pytest.raises(NotImplementedError) as e:
        EV.PerformanceMeter(config, E.VMIN, E.VMAX)
    bad = [k for k in config if k in ("PSNR", "Slope", "SSIM", "RMSE", "MAE", "Foo")][-1 if "Foo" in config else 0]
    assert bad in str(e.value)
    if config.get(bad) and config[bad].get("package"):
        assert config[bad]["package"] in str(e.value)


def test_metric_with_its_own_crop_is_refused():
    with pytest.raises(NotImplementedError):
        EV.PerformanceMeter({"RMSE": {"package": "local", "border": 0.1}}, E.VMIN, E.VMAX, border=0.05)
    EV.PerformanceMeter({"RMSE": {"package": "local", "border": 0.05, "min": E.VMIN, "max": E.VMAX}}, E.VMIN, E.VMAX, border=0.05)


def test_validate_results_recorded_rows(g12):
    rows = json.loads(str(g12["validate_rows"]))
    assert len(rows) >= 40 and any(r["raises"] for r in rows) and any(r["better"] for r in rows)
    for r in rows:
        if r["raises"]:
            with pytest.raises(KeyError):
                EV.validate_results(dict(r["current"]), dict(r["reference"]), r["best_metric"])
            continue
        better, kept = EV.validate_results(dict(r["current"]), dict(r["reference"]), r["best_metric"])
        assert better is r["better"] and kept == r["kept"], r
    with pytest.raises(AssertionError):
        EV.validate_results({"RMSE": 1.0}, {"PSNR": 1.0})


def test_do_eval_recorded_rows(g12):
    args, res = g12["do_eval_args"], g12["do_eval_result"]
    assert len(args) == len(res) > 100 and res.any() and not res.all()
    for a, r in zip(args.tolist(), res.tolist()):
        epochs, cur, start, warm, interval, vstart = a
        assert EV.do_eval(epochs, cur, start, warm, None if interval < 0 else interval, vstart) is bool(r), a
