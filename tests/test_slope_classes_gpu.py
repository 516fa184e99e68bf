"""K22 on the MI355X: the slope-class plane (jspsr_slope_classes) against tests/slope_ref.py, a numpy float32 restatement in
the kernel's operation order with np.pad(mode="edge") per scene.  The labels are compared with np.array_equal: there is no
tolerance and no share of exceptions.  One end-to-end test: `summarise_by_class(labels=slope_class_plane(...))` against the
host route (copy, boolean indexing, `summary_ref.scores`)."""
import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import summary as S
from tests import slope_ref
from tests import summary_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VMAX = 933.0
P = dict(elev_min=-80, elev_max=933, elev_log=True)


def store(rasters):
    return D.DeviceScenes(lr_dem=[a[..., None] for a in rasters], hr_dem=[a[..., None] for a in rasters], relative=True, device=DEV, **P)


def terrain(shape, seed, step=None):
    """Metres between 100 and 600 with slopes from flat to steep; step: quantised to multiples of it."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    z = 350 + 120 * np.sin(x / 7.0 + rs.rand()) * np.cos(y / 5.0 + rs.rand()) + 0.03 * (x - shape[1] / 2) ** 2 + rs.uniform(-1, 1, shape)
    z = np.clip(z, 100, 600)
    if step:
        z = np.round(z / step) * step
    return z.astype(np.float32)


def plane_of(rasters, edges, cell, valids=None, source="hr_dem"):
    scenes = store(rasters)
    before = _lib.load().jspsr_launch_count(b"slope_classes")
    valid = None if valids is None else torch.from_numpy(np.concatenate([v.reshape(-1) for v in valids]).astype(np.uint8)).to(DEV)
    got = S.slope_class_plane(scenes, edges, cell, source=source, valid=valid)
    assert _lib.load().jspsr_launch_count(b"slope_classes") == before + 1                       # one launch
    assert got.dtype == torch.uint8 and got.dim() == 1 and got.device == scenes.store["hr_dem"].device
    assert got.numel() == sum(h * w for h, w in scenes.shapes)
    return got.cpu().numpy()


EDGES = [2.0, 5.0, 15.0, 30.0, 45.0]


def test_random_metre_rasters():
    z = [terrain((61, 83), 1)]
    got = plane_of(z, EDGES, 10.0)
    want = slope_ref.plane(z, slope_ref.thresholds(EDGES, 10.0))
    assert np.array_equal(got, want)
    assert len(np.unique(want)) >= 5 and want.max() <= len(EDGES)


def test_integer_valued_rasters():
    z = [terrain((45, 52), 2, step=1.0)]
    for cell in (1.0, 30.0):
        assert np.array_equal(plane_of(z, EDGES, cell), slope_ref.plane(z, slope_ref.thresholds(EDGES, cell)))


def test_two_scenes_in_one_store_and_no_tap_crosses_between_them():
    z = [terrain((37, 53), 3), terrain((64, 40), 4) + 150]                        # a step of 150 m between the scenes
    got = plane_of(z, EDGES, 10.0)
    want = slope_ref.plane(z, slope_ref.thresholds(EDGES, 10.0))                  # each scene padded on its own
    assert np.array_equal(got, want)
    joined = slope_ref.labels(np.concatenate([z[0].reshape(-1), z[1].reshape(-1)]).reshape(1, -1), slope_ref.thresholds(EDGES, 10.0))
    assert not np.array_equal(joined.reshape(-1), want)                           # the rows of one flat raster would differ


def test_scenes_of_one_pixel_and_of_one_row():
    z = [np.array([[321.5]], np.float32), terrain((1, 9), 5), terrain((9, 1), 6), terrain((2, 2), 7)]
    got = plane_of(z, EDGES, 1.0)
    assert np.array_equal(got, slope_ref.plane(z, slope_ref.thresholds(EDGES, 1.0)))
    assert got[0] == 0                                                            # one pixel: every tap is the pixel itself, p = 0


def test_a_slope_on_the_edge_belongs_to_the_upper_class():
    z = [np.tile(np.arange(12, dtype=np.float32) + 200, (7, 1))]                   # z = x, cell = 1: 45 degrees
    thr = S.slope_thresholds([45.0], 1.0)
    assert thr[0] == np.float32(64.0)
    got = plane_of(z, [45.0], 1.0).reshape(7, 12)
    assert np.array_equal(got, slope_ref.labels(z[0], thr))
    assert (got[:, 1:-1] == 1).all() and (got[:, [0, -1]] == 0).all()             # inside p = 64 meets t = 64.0; the clamped columns see p = 16


def test_holes_in_the_validity_plane():
    z = [terrain((40, 44), 8), terrain((21, 33), 9)]
    valids = [np.ones(a.shape, bool) for a in z]
    holes = [[(0, 0), (5, 7), (20, 43), (39, 20), (30, 30)], [(10, 10), (20, 32)]]
    for v, hs in zip(valids, holes):
        for y, x in hs:
            v[y, x] = False
    got = plane_of(z, EDGES, 10.0, valids)
    want = slope_ref.plane(z, slope_ref.thresholds(EDGES, 10.0), valids)
    assert np.array_equal(got, want)
    off = 0
    for a, hs in zip(z, holes):
        lab = got[off:off + a.size].reshape(a.shape)
        mark = np.zeros(a.shape, bool)
        for y, x in hs:
            mark[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
        assert (lab[mark] == 255).all() and (lab[~mark] != 255).all()             # 255 exactly on the 3 x 3 neighbourhood of every hole
        off += a.size


def test_a_nan_under_a_valid_tap():
    z = [terrain((30, 31), 10)]
    scenes = store(z)
    scenes.store["hr_dem"][5 * 31 + 6] = float("nan")
    scenes.store["hr_dem"][29 * 31 + 30] = float("inf")
    host = z[0].copy()
    host[5, 6], host[29, 30] = np.nan, np.inf
    valid = torch.ones(30 * 31, dtype=torch.uint8, device=DEV)
    got = S.slope_class_plane(scenes, EDGES, 10.0, valid=valid).cpu().numpy().reshape(30, 31)
    assert np.array_equal(got, slope_ref.labels(host, slope_ref.thresholds(EDGES, 10.0), np.ones((30, 31), bool)))
    # the centre tap e is in neither sum: its own label survives, its eight neighbours' do not
    # (the infinity in the corner makes p = inf there, the top class, not a NaN)
    assert (got[4:7, 5:8] == 255).sum() == 8 and got[5, 6] != 255 and (got == 255).sum() == 8 and got[29, 30] == len(EDGES)
    assert np.array_equal(S.slope_class_plane(scenes, EDGES, 10.0).cpu().numpy().reshape(30, 31), got)   # and without a plane


def test_thirty_one_edges_and_the_low_resolution_raster():
    z = [terrain((50, 57), 11)]
    edges = list(np.linspace(0.0, 75.0, 31))
    got = plane_of(z, edges, 10.0)
    want = slope_ref.plane(z, slope_ref.thresholds(edges, 10.0))
    assert np.array_equal(got, want) and want.min() >= 1 and want.max() >= 20     # edge 0: t = 0 <= p always
    assert np.array_equal(plane_of(z, [], 10.0), np.zeros(z[0].size, np.uint8))   # no edge: one class
    assert np.array_equal(plane_of(z, EDGES, 10.0, source="lr_dem"), slope_ref.plane(z, slope_ref.thresholds(EDGES, 10.0)))


def test_slope_thresholds_are_the_formula_in_double():
    import math
    for cell in (1.0, 10.0, 30.0):
        for e, t in zip(EDGES, S.slope_thresholds(EDGES, cell)):
            assert t.tobytes() == np.float32((8.0 * cell * math.tan(e * math.pi / 180.0)) ** 2).tobytes()


def test_summarise_by_class_over_slope_classes_end_to_end():
    rs = np.random.RandomState(12)
    gts = [terrain((48, 60), 13), terrain((40, 52), 14)]
    lrs = [g + rs.uniform(-5, 5, g.shape).astype(np.float32) for g in gts]
    scenes = D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, device=DEV, **P)
    preds = [(g + rs.standard_normal(g.shape) * 1.5).astype(np.float32) for g in gts]
    edges, cell, b = [5.0, 15.0, 30.0], 10.0, 1
    names = ["flat", "gentle", "steep", "cliff"]
    labels = S.slope_class_plane(scenes, edges, cell)
    table = S.summarise_by_class(scenes, preds, labels, names, baselines={"COP30": "lr_dem"}, value_max=VMAX, border=0.05, patch_size=32)
    cls = np.concatenate([R.crop(slope_ref.labels(g, slope_ref.thresholds(edges, cell)), b, g.shape) for g in gts]).astype(np.int64)
    assert len(np.unique(cls)) == 4
    for name, rasters in (("SR", preds), ("COP30", lrs)):
        e = R.errors(rasters, gts, b)                                             # the host route: copy, boolean indexing, numpy
        for k, cname in enumerate(names):
            got, want = table[name][cname], R.scores(e[cls == k], VMAX)
            assert got["N"] == int((cls == k).sum()) and got["share"] == got["N"] / cls.size
            R.check_row(np.array([got[c] for c in R.COLUMNS] + list(want["brackets"])), want, f"{name} {cname}")
