"""The host path of jspsr_amd.summary (the formulas of K12 as numpy / torch operators) against the numpy restatement of
summarise_evaluation (tests/summary_ref.py), and the rank helper the device's segment table is made by."""
import numpy as np
import pytest
import torch

from jspsr_amd import data as D
from jspsr_amd import summary as S
from tests import summary_ref as R

VMAX = 933.0
SHAPES = [(40, 56), (37, 53), (64, 64)]
PATCH, BORDER = 30, 0.1            # int(30 * 0.1) = 3 pixels per side


def quantised_scenes(shapes=SHAPES, seed=3):
    """Ground truth, an input DEM and a prediction on a 1/128 m grid (every difference is exact in fp32): heavy ties, zeros,
    both signs."""
    rs = np.random.RandomState(seed)
    gts, lrs, srs = [], [], []
    for h, w in shapes:
        gt = np.round(rs.uniform(100, 600, (h, w)) * 128) / 128
        lr = gt + rs.randint(-400, 401, (h, w)) / 128
        sr = gt + rs.randint(-6, 7, (h, w)) / 128
        sr[:4] = gt[:4]
        gts.append(gt.astype(np.float32))
        lrs.append(lr.astype(np.float32))
        srs.append(sr.astype(np.float32))
    return gts, lrs, srs


def host_store(gts, lrs):
    return D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], elev_min=0.0, elev_max=1000.0,
                          device="cpu")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 20, 21, 22, 101, 4096, 103_684])
def test_segment_ranks(n):
    m0, m1, l0, l1, g = S.segment_ranks(n)
    assert (m0, m1) == ((n - 1) // 2, n // 2) and m1 - m0 == (0 if n % 2 else 1)
    assert 0 <= l0 <= l1 <= n - 1 and l1 - l0 <= 1 and 0.0 <= g < 1.0
    assert (m0, m1, l0, l1) == R.ranks(n)
    a = np.sort(np.random.RandomState(n).standard_normal(n))
    assert a[l0] + (a[l1] - a[l0]) * g == pytest.approx(np.percentile(a, 95), rel=1e-12, abs=1e-12)
    assert (a[m0] + a[m1]) / 2 == np.median(a)


def test_segment_ranks_small_and_integer_index():
    assert S.segment_ranks(1) == (0, 0, 0, 0, 0.0)
    assert S.segment_ranks(2)[:4] == (0, 1, 0, 1) and S.segment_ranks(2)[4] == pytest.approx(0.95)
    assert S.segment_ranks(21) == (10, 10, 19, 20, 0.0)          # 0.95 * 20 sits on an integer
    with pytest.raises(ValueError):
        S.segment_ranks(0)


def test_summarise_host_matches_restatement():
    gts, lrs, srs = quantised_scenes()
    scenes = host_store(gts, lrs)
    fab = [g + np.float32(0.5) for g in gts]
    pooled, means, per_scene = S.summarise(scenes, srs, baselines={"COP30": "lr_dem", "FABDEM": fab}, value_max=VMAX, border=BORDER,
                                           patch_size=PATCH, online=True)
    off, onl, per = R.summarise(gts, {"SR": srs, "COP30": lrs, "FABDEM": fab}, 3, VMAX)
    assert list(pooled) == ["SR", "COP30", "FABDEM"]
    for name in pooled:
        for k in R.COLUMNS:
            assert pooled[name][k] == pytest.approx(float(off[name][k]), rel=2e-7, abs=0), (name, k)
            assert means[name][k] == pytest.approx(onl[name][k], rel=2e-7, abs=1e-9), (name, k)
        assert np.float32(pooled[name]["Median"]) == off[name]["Median"]
        for i, sid in enumerate(scenes.ids):
            assert np.float32(per_scene[name][sid]["Median"]) == per[name][i]["Median"]
    assert S.summarise(scenes, srs, baselines={"COP30": "lr_dem", "FABDEM": fab}, value_max=VMAX, border=BORDER, patch_size=PATCH) == pooled
    # a prediction that already has the cropped size is taken whole (utils.py:1300-1306)
    cropped = [a[3:-3, 3:-3] for a in srs]
    assert S.summarise(scenes, cropped, value_max=VMAX, border=BORDER, patch_size=PATCH)["SR"] == pooled["SR"]


def test_scores_pooled_host_rows_and_segments():
    gts, lrs, srs = quantised_scenes([(64, 64)] * 3)
    gt, lr, sr = (torch.from_numpy(np.stack(a)) for a in (gts, lrs, srs))
    rows = S.scores_pooled([sr, lr], gt, value_max=VMAX)
    assert rows.shape == (2, 1, len(S.ROW))
    for c, cand in enumerate((srs, lrs)):
        R.check_row(rows[c, 0].numpy(), R.scores(R.errors(cand, gts, 0), VMAX), f"cand {c}")
    segs = [[(0, 3, 3, 58, 58)], [(1, 0, 0, 64, 64), (2, 5, 7, 11, 13)]]
    rows = S.scores_pooled(sr, gt, segments=segs, value_max=VMAX)
    e = [srs[i] - gts[i] for i in range(3)]
    R.check_row(rows[0, 0].numpy(), R.scores(e[0][3:61, 3:61].flatten(), VMAX), "seg 0")
    R.check_row(rows[0, 1].numpy(), R.scores(np.concatenate((e[1].flatten(), e[2][5:16, 7:20].flatten())), VMAX), "seg 1")


@pytest.mark.parametrize("full,k,n,border,lg", [(70, 32, 9, 0.05, True), (48, 32, 4, 0.1, False), (32, 32, 1, 0.05, True)])
def test_assembly_host_equals_composition(full, k, n, border, lg):
    rs = np.random.RandomState(full + n)
    n_sc = 3
    gts = [rs.uniform(150, 400, (full, full)).astype(np.float32) for _ in range(n_sc)]
    lrs = [g + rs.uniform(-5, 5, g.shape).astype(np.float32) for g in gts]
    scenes = D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, elev_min=-80,
                            elev_max=933, elev_log=lg, device="cpu")
    tiles = torch.from_numpy(rs.uniform(-0.1, 1.1, (n_sc * n, 1, k, k)).astype(np.float32))
    c = S.ScenePredictions(scenes, k, n, border=border)
    metas = [{"id": scenes.ids[i // n]} for i in range(n_sc * n)]
    for lo in range(0, n_sc * n, 10):                              # scenes straddle the batches
        assert not c.complete
        c.add(tiles[lo:lo + 10], metas[lo:lo + 10])
    assert c.complete
    got = c.rasters()
    for i, sid in enumerate(scenes.ids):
        want = R.assemble(tiles[i * n:(i + 1) * n], scenes.base[i], full, border, -80, 933, lg).numpy()
        assert got[sid].shape == want.shape == c.shape
        assert got[sid].tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        c.add(tiles[:1], metas[:1])                                # more tiles than the scenes hold
    c.reset()
    with pytest.raises(ValueError):
        c.add(tiles[:2], [{"id": "nobody"}] * 2)


def test_nan_makes_the_rows_scores_nan():
    gt = torch.zeros(2, 16, 16)
    cand = torch.from_numpy(np.random.RandomState(0).standard_normal((2, 16, 16)).astype(np.float32))
    cand[1, 3, 4] = float("nan")
    rows = S.scores_pooled(cand, gt, segments=[[(0, 0, 0, 16, 16)], [(1, 0, 0, 16, 16)]], value_max=VMAX).numpy()
    assert np.isfinite(rows[0, 0]).all()
    assert np.isnan(rows[0, 1, :5]).all()
    with np.errstate(all="ignore"):
        assert np.isnan(np.median(cand[1].numpy()))                # numpy's rule


def test_psnr_is_inf_at_zero_error():
    gt = torch.rand(1, 9, 9)
    row = S.scores_pooled(gt.clone(), gt, value_max=VMAX)[0, 0].numpy()
    assert row[4] == np.inf and (row[:4] == 0).all() and (row[5:] == 0).all()


def test_bad_tables_are_refused():
    gt = torch.zeros(1, 8, 8)
    with pytest.raises(ValueError):
        S.scores_pooled(gt, gt, segments=[[(0, 0, 0, 0, 8)]])       # an empty window
    with pytest.raises(ValueError):
        S.scores_pooled(gt, gt, segments=[[(0, 4, 4, 8, 8)]])       # leaves the tensor
    with pytest.raises(ValueError):
        S.scores_pooled([gt] * 9, gt)
    with pytest.raises(ValueError):
        S.scores_pooled(gt, gt, segments=[[(0, 0, 0, 8, 8)], []])   # a segment without windows


def test_window_table_rows():
    """The rows K12, K21 and K22 read, written out: word 3 runs over h * w, the slots of candidates 2..7 stay 0, word 0 is
    the segment or 0."""
    windows = [(1, 3, 5, (7, 11), [(2, 5), (40, 9)]),
               (0, 2, 4, (100, 6), [(0, 4), (8, 13)]),
               (1, 1, 6, (50, 6), [(17, 6), (3, 7)])]
    pad = [0] * 12
    rows = [[1, 3, 5, 0, 7, 11, 2, 5, 40, 9] + pad,
            [0, 2, 4, 15, 100, 6, 0, 4, 8, 13] + pad,
            [1, 1, 6, 23, 50, 6, 17, 6, 3, 7] + pad]
    kept = S._window_table(windows, True)
    assert kept.dtype == np.int64 and kept.shape == (3, 22)
    assert kept.tolist() == rows
    assert S._window_table(windows, False).tolist() == [[0] + r[1:] for r in rows]
