"""Scores by terrain class (K22) without a GPU: the host paths of `stratified_rows`, `scores_by_class` and
`summarise_by_class` against the restatement on the host-compacted errors of every class (tests/summary_ref.py:
`scores(e[class], value_max)`, `check_row`); the slope restatement (tests/slope_ref.py) against a float64 evaluation of the
slope in degrees, on rasters on which no pixel's slope lies within 1e-3 degrees of an edge; `slope_thresholds` against the
formula; the argument refusals in Python and at the C entries before any launch; header, binding and library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import summary as S
from tests import slope_ref
from tests import summary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMAX = 933.0
ENTRIES = {"jspsr_strata_workspace_bytes": 3, "jspsr_strata_forward": 18, "jspsr_slope_classes": 10}
P = dict(elev_min=-80, elev_max=933, elev_log=True)


def check_classes(rows, counts, errors, cls, n_classes, tag):
    """rows (n_cand, n_classes, 11), counts (n_classes,) against the restatement: errors[c] the pooled float32 errors of
    candidate c, cls the class of every pooled element (anything >= n_classes: none)."""
    assert rows.shape == (len(errors), n_classes, 11) and counts.shape == (n_classes,)
    for k in range(n_classes):
        assert counts[k] == int((cls == k).sum()), (tag, k)
        for c, e in enumerate(errors):
            ek = e[cls == k]
            if ek.size == 0:
                assert np.isnan(rows[c, k]).all(), (tag, c, k)
            else:
                R.check_row(rows[c, k], R.scores(ek, VMAX), f"{tag} cand {c} class {k} n {ek.size}")


# ---- host paths ------------------------------------------------------------------------------------------------------
def small_case():
    rs = np.random.RandomState(22)
    gt = rs.uniform(100, 600, (2, 14, 19)).astype(np.float32)
    cands = [(gt + rs.standard_normal(gt.shape) * s).astype(np.float32) for s in (0.5, 6.0)]
    labels = rs.randint(0, 4, gt.shape).astype(np.uint8)
    labels[labels == 2] = 0                                                       # class 2 is empty
    labels[0, 3, :] = 255
    labels[1, :, 4] = 7                                                           # >= n_classes: no class
    valid = rs.rand(*gt.shape) < 0.7
    none = (labels >= 4) | ~valid
    for c in cands:                                                               # what has no class must not matter
        c[none] = -32767.0
    gt[0, 5, 5], labels[0, 5, 5] = np.nan, 255
    return gt, cands, labels, valid


def test_scores_by_class_host_path_matches_the_compacted_restatement():
    gt, cands, labels, valid = small_case()
    rows, counts = S.scores_by_class([torch.from_numpy(c) for c in cands], torch.from_numpy(gt), torch.from_numpy(labels), 4,
                                     value_max=VMAX, valid=torch.from_numpy(valid))
    assert rows.dtype == torch.float32 and counts.dtype == torch.int64
    cls = np.where(valid, labels, 255).reshape(-1)
    with np.errstate(invalid="ignore"):
        errors = [(c - gt).reshape(-1) for c in cands]
    check_classes(rows.numpy(), counts.numpy(), errors, cls, 4, "scores_by_class")
    assert counts[2] == 0 and counts.sum() == (cls < 4).sum()
    plain, n_plain = S.scores_by_class(torch.from_numpy(cands[0]), torch.from_numpy(gt), torch.from_numpy(labels), 4, value_max=VMAX)
    check_classes(plain.numpy(), n_plain.numpy(), errors[:1], labels.reshape(-1), 4, "no valid")


def test_stratified_rows_host_path_with_pitched_windows():
    gt, cands, labels, valid = small_case()
    wins = [(1, 2, 3, 9, 11), (0, 0, 0, 14, 19), (1, 12, 0, 2, 19)]               # (plane, y0, x0, h, w)
    H, W = gt.shape[1:]
    windows = [(5, h, w, ((p * H + y) * W + x, W), [((p * H + y) * W + x, W)] * 2) for p, y, x, h, w in wins]   # the segment entry is not read
    flat = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    rows, counts = S.stratified_rows([flat(c) for c in cands], flat(gt), windows, flat(labels), 3, VMAX, valid=flat(valid.astype(np.uint8)))
    cut = lambda a: np.concatenate([a[p, y:y + h, x:x + w].reshape(-1) for p, y, x, h, w in wins])
    cls = np.where(cut(valid), cut(labels), 255)
    with np.errstate(invalid="ignore"):
        errors = [cut(c) - cut(gt) for c in cands]
    check_classes(rows.numpy(), counts.numpy(), errors, cls, 3, "pitched")         # label 3 is >= n_classes here: ignored


def cpu_scenes(n_sc=3, full=20, seed=5):
    rs = np.random.RandomState(seed)
    gts = [rs.uniform(150, 400, (full, full)).astype(np.float32) + 37 * i for i in range(n_sc)]
    lrs = [g + rs.uniform(-5, 5, g.shape).astype(np.float32) for g in gts]
    scenes = D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, device="cpu", **P)
    return scenes, gts, lrs, rs


@pytest.mark.parametrize("form", ["list", "flat"])
def test_summarise_by_class_host_path(form):
    scenes, gts, lrs, rs = cpu_scenes()
    b = 2                                                                         # int(16 * 0.125)
    names = ["water", "forest", "built", "bare"]
    labs = [rs.randint(0, 3, (20, 20)).astype(np.uint8) for _ in gts]             # "bare" stays empty
    labs[1][::3] = 255
    valids = [rs.rand(20, 20) < 0.8 for _ in gts]
    preds = [(g + rs.standard_normal(g.shape)).astype(np.float32) for g in gts]
    for p, v, l in zip(preds, valids, labs):
        p[~v | (l == 255)] = -32767.0
    given = [preds[0], preds[1][b:-b, b:-b].copy(), preds[2]]                     # whole and cropped rasters
    labels = labs if form == "list" else torch.from_numpy(np.concatenate([l.reshape(-1) for l in labs]))
    table = S.summarise_by_class(scenes, given, labels, names, baselines={"COP30": "lr_dem"}, value_max=VMAX, border=0.125,
                                 patch_size=16, valid=valids)
    assert list(table) == ["SR", "COP30"] and all(list(t) == names for t in table.values())
    cls = np.concatenate([np.where(R.crop(v, b, v.shape) != 0, R.crop(l, b, l.shape), 255) for v, l in zip(valids, labs)]).astype(np.int64)
    for name, rasters in (("SR", preds), ("COP30", lrs)):
        e = R.errors(rasters, gts, b)
        for k, cname in enumerate(names):
            got, ek = table[name][cname], e[cls == k]
            assert got["N"] == ek.size and set(got) == set(R.COLUMNS) | {"N", "share"}
            assert got["share"] == ek.size / int((cls < 4).sum())
            if ek.size == 0:
                assert cname == "bare" and all(np.isnan(got[c]) for c in R.COLUMNS)
                continue
            want = R.scores(ek, VMAX)
            R.check_row(np.array([got[c] for c in R.COLUMNS] + list(want["brackets"])), want, f"{name} {cname}")
        assert abs(sum(t["share"] for t in table[name].values()) - 1.0) < 1e-12
    nothing = S.summarise_by_class(scenes, given, [np.full((20, 20), 255, np.uint8)] * 3, ["a"], value_max=VMAX, border=0.125, patch_size=16)
    assert nothing["SR"]["a"]["N"] == 0 and np.isnan(nothing["SR"]["a"]["share"]) and np.isnan(nothing["SR"]["a"]["RMSE"])


# ---- slope classes ---------------------------------------------------------------------------------------------------
EDGES, CELL = [2.0, 5.0, 15.0, 30.0], 10.0


def slope_raster():
    """Eighths of a metre (every Sobel sum is exact in float32) with slopes from flat to steep, and no pixel's slope within
    1e-3 degrees of an edge: the first seed that has the property, searched deterministically."""
    for seed in range(50):
        rs = np.random.RandomState(seed)
        y, x = np.mgrid[0:41, 0:47]
        z = 300 + 60 * np.sin(x / 6.0) * np.cos(y / 9.0) + 0.02 * (x - 20) ** 2 + rs.uniform(-0.5, 0.5, x.shape)
        z = (np.round(z * 8) / 8).astype(np.float32)
        deg = slope_ref.degrees(z, CELL)
        if min(np.abs(deg - e).min() for e in EDGES) > 1e-3:
            return z, deg
    raise AssertionError("no raster found")


def test_slope_ref_against_the_slope_in_degrees():
    z, deg = slope_raster()
    assert min(np.abs(deg - e).min() for e in EDGES) > 1e-3                       # the precondition
    want = sum((deg >= e).astype(np.int64) for e in EDGES)
    got = slope_ref.labels(z, slope_ref.thresholds(EDGES, CELL))
    assert np.array_equal(got, want)
    assert set(np.unique(got)) == {0, 1, 2, 3, 4}                                 # every class occurs
    scenes = D.DeviceScenes(lr_dem=[z[..., None]], hr_dem=[z[..., None]], relative=True, device="cpu", **P)
    plane = S.slope_class_plane(scenes, EDGES, CELL)                              # the package's host path
    assert plane.dtype == torch.uint8 and np.array_equal(plane.numpy(), got.reshape(-1))
    valid = np.ones(z.shape, bool)
    valid[7, 9] = valid[0, 0] = False
    holes = S.slope_class_plane(scenes, EDGES, CELL, valid=[valid]).numpy().reshape(z.shape)
    assert np.array_equal(holes, slope_ref.labels(z, slope_ref.thresholds(EDGES, CELL), valid))
    assert (holes[6:9, 8:11] == 255).all() and (holes[0:2, 0:2] == 255).all() and (holes == 255).sum() == 13


def test_slope_thresholds_are_the_formula_in_double():
    edges = [0.0, 0.5, 1.0, 15.0, 45.0, 60.0, 89.9]
    for cell in (1.0, 8.0, 30.0, 0.25):
        got = S.slope_thresholds(edges, cell)
        assert got.dtype == np.float32 and got.shape == (len(edges),)
        for e, t in zip(edges, got):
            assert t.tobytes() == np.float32((8.0 * cell * math.tan(e * math.pi / 180.0)) ** 2).tobytes(), (e, cell)
        assert np.array_equal(got, slope_ref.thresholds(edges, cell))
    assert S.slope_thresholds([45.0], 1.0)[0] == np.float32(64.0)                 # z = x, cell = 1: p = 64 meets it
    assert S.slope_thresholds([], 1.0).shape == (0,)
    assert len(S.slope_thresholds(np.linspace(0, 89, 31), 2.0)) == 31


# ---- argument errors -------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    gt = torch.zeros(64)
    win = [(0, 8, 8, (0, 8), [(0, 8)])]
    ok = torch.zeros(64, dtype=torch.uint8)
    rows, counts = S.stratified_rows([gt], gt, win, ok, 2, VMAX)
    assert rows.shape == (1, 2, 11) and counts.tolist() == [64, 0]
    for bad in (ok.bool(), ok.float(), ok[:63], ok.view(8, 8), torch.zeros(128, dtype=torch.uint8)[::2], np.zeros(64, np.uint8)):
        with pytest.raises(ValueError, match="labels"):
            S.stratified_rows([gt], gt, win, bad, 2, VMAX)
    for bad in (0, 33, -1, 2.0, None):
        with pytest.raises(ValueError, match="n_classes"):
            S.stratified_rows([gt], gt, win, ok, bad, VMAX)
    with pytest.raises(ValueError, match="valid"):
        S.stratified_rows([gt], gt, win, ok, 2, VMAX, valid=ok[:63])
    with pytest.raises(ValueError, match="candidates"):
        S.stratified_rows([gt] * 9, gt, [(0, 8, 8, (0, 8), [(0, 8)] * 9)], ok, 2, VMAX)
    g2 = gt.view(1, 8, 8)
    for bad in (torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.bool)):
        with pytest.raises(ValueError, match="labels"):
            S.scores_by_class(g2, g2, bad, 2)
    with pytest.raises(ValueError, match="valid"):
        S.scores_by_class(g2, g2, ok.view(1, 8, 8), 2, valid=torch.ones(8, 8, dtype=torch.bool))
    scenes, gts, lrs, rs = cpu_scenes()
    kw = dict(value_max=VMAX, border=0.125, patch_size=16)
    lab = [np.zeros((20, 20), np.uint8)] * 3
    for bad in (lab[:2], [np.zeros((20, 19), np.uint8)] * 3, [np.zeros((20, 20), np.int64)] * 3, torch.zeros(1199, dtype=torch.uint8),
                torch.zeros(1200, dtype=torch.int64), torch.zeros(3 * 16 * 16, dtype=torch.uint8)):   # the last: the cropped layout
        with pytest.raises(ValueError, match="labels"):
            S.summarise_by_class(scenes, lrs, bad, ["a", "b"], **kw)
    for bad in ([], ["a"] * 2, [str(i) for i in range(33)]):
        with pytest.raises(ValueError, match="class names"):
            S.summarise_by_class(scenes, lrs, lab, bad, **kw)
    for edges, cell in (([5.0, 5.0], 1.0), ([15.0, 5.0], 1.0), ([-1.0], 1.0), ([90.0], 1.0), ([float("nan")], 1.0), ([5.0], 0.0),
                        ([5.0], -2.0), ([5.0], float("inf")), (list(np.linspace(0, 80, 32)), 1.0)):
        with pytest.raises(ValueError, match="slope_thresholds"):
            S.slope_class_plane(scenes, edges, cell)
    with pytest.raises(ValueError, match="source"):
        S.slope_class_plane(scenes, [5.0], 1.0, source="image")
    with pytest.raises(ValueError, match="valid"):
        S.slope_class_plane(scenes, [5.0], 1.0, valid=torch.ones(1199, dtype=torch.uint8))


def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN with a message that names the entry, before a launch (safe without a GPU: no device
    pointer is dereferenced, the host arrays are real)."""
    lib = _lib.load()
    x, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    census = (b"strata_prepare", b"strata_select", b"slope_classes")
    before = {n: lib.jspsr_launch_count(n) for n in census}
    ptrs, numel = (ctypes.c_void_p * 8)(*[4096] * 8), (ctypes.c_longlong * 8)(*[64] * 8)

    def call(cands=ptrs, n_cand=1, gt=x, gt_numel=64, labels=x, labels_numel=64, n_classes=3, valid=None, valid_numel=0, windows=x,
             n_windows=1, total=64, out=x, counts=x, ws=x):
        return lib.jspsr_strata_forward(cands, numel, n_cand, gt, gt_numel, labels, labels_numel, n_classes, valid, valid_numel, windows,
                                        n_windows, total, VMAX, out, counts, ws, None)

    def message():
        return lib.jspsr_last_error().decode()

    for kw in (dict(cands=None), dict(gt=None), dict(labels=None), dict(counts=None), dict(windows=None), dict(out=None), dict(ws=None),
               dict(n_cand=0), dict(n_cand=9), dict(n_classes=0), dict(n_classes=33), dict(n_windows=0), dict(total=0), dict(gt_numel=0),
               dict(labels_numel=63), dict(valid=x, valid_numel=65), dict(total=2 ** 32)):
        assert call(**kw) == -1 and "strata_forward" in message(), kw
    assert call(labels_numel=63) == -1 and "label plane" in message()
    assert call(n_classes=33) == -1 and "n_classes" in message()
    nulls = (ctypes.c_void_p * 8)(4096, None, *[4096] * 6)
    assert call(cands=nulls, n_cand=2) == -1 and "candidate 1" in message()
    for kw in (dict(gt=odd), dict(out=odd), dict(ws=ctypes.c_void_p(4104)), dict(counts=ctypes.c_void_p(4100))):
        assert call(**kw) == -2 and "aligned" in message() and "strata_forward" in message(), kw
    size = lib.jspsr_strata_workspace_bytes
    assert size(0, 1, 64) == 0 and size(9, 1, 64) == 0 and size(1, 0, 64) == 0 and size(1, 33, 64) == 0 and size(1, 1, 2 ** 32) == 0
    assert size(1, 1, 0) == 0
    for n_cand, n_classes, total in ((1, 1, 64), (3, 5, 100000), (8, 32, 4096 * 4096)):
        runs = (total + S.CHUNK - 1) // S.CHUNK
        floor = n_cand * total * 4 + total + n_cand * runs * n_classes * 8 + n_cand * n_classes * (6 * 1024 + 64)   # e, classes, sums, one replica
        assert floor <= size(n_cand, n_classes, total) <= floor + 15 * n_cand * n_classes * 6 * 1024 + 128, (n_cand, n_classes, total)

    thr = (ctypes.c_float * 31)(*[float(i) for i in range(31)])

    def slope(z=x, pixels=64, scenes=x, n_scenes=1, t=thr, n_thr=3, valid=None, valid_numel=0, out=x):
        return lib.jspsr_slope_classes(z, pixels, scenes, n_scenes, t, n_thr, valid, valid_numel, out, None)

    for kw in (dict(z=None), dict(scenes=None), dict(out=None), dict(pixels=0), dict(n_scenes=0), dict(n_thr=32), dict(n_thr=-1),
               dict(t=None), dict(valid=x, valid_numel=63), dict(t=(ctypes.c_float * 3)(1.0, 3.0, 2.0)),
               dict(t=(ctypes.c_float * 3)(-1.0, 3.0, 4.0)), dict(t=(ctypes.c_float * 3)(1.0, float("nan"), 4.0))):
        assert slope(**kw) == -1 and "slope_classes" in message(), kw
    assert slope(z=odd) == -2 and "aligned" in message()
    assert before == {n: lib.jspsr_launch_count(n) for n in census}


def test_header_library_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert "K22 (ABI v25, additive)" in hdr
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\b(?:int|size_t)\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    assert _lib.load().jspsr_abi_version() == _lib.ABI_VERSION
    assert all(callable(getattr(S, name)) for name in ("stratified_rows", "scores_by_class", "slope_class_plane", "slope_thresholds",
                                                       "summarise_by_class"))
