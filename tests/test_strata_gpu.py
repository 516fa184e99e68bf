"""K22 on the MI355X: scores by terrain class (jspsr_strata_forward) against two references.

Reference 1 (host): for every class and candidate `summary_ref.check_row(row, summary_ref.scores(e[class], VMAX))` on the
host-compacted errors -- the project's K12 tolerance (the six bracketing order statistics equal as values, Median bit-equal,
NMAD / LE95 / PSNR within 1 fp32 ulp of the float64 value, RMSE within 2) -- and the counts compared with ==.
Reference 2 (device): for every class the six bracketing columns and the Median are bit-equal (`tobytes()`) to the loop K22
replaces, `scores_pooled(..., valid=(labels == c) & valid)`.

What belongs to no class (a label of 255, a label >= n_classes, a masked pixel) changes no byte of the output whatever the
rasters hold there; one counted NaN makes one row's five scores NaN and leaves every other row byte-identical; a row does not
depend on the other classes' values, on the number of candidates or on the run; the number of launches does not depend on
n_classes."""
import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import summary as S
from tests import summary_ref as R
from tests.test_summary_valid_gpu import errors_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VMAX = 933.0
CENSUS = (b"strata_prepare", b"strata_select")
EXACT = [1, 5, 6, 7, 8, 9, 10]                # Median and the six brackets


def launches(*names):
    return sum(_lib.load().jspsr_launch_count(n) for n in names)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def by_class(cands, gt, labels, n_classes, valid=None):
    """numpy (planes, H, W) arrays -> ((n_cand, n_classes, 11) rows, (n_classes,) counts) from the device."""
    cands = [cands] if isinstance(cands, np.ndarray) else cands
    rows, counts = S.scores_by_class([dev(c) for c in cands], dev(gt), dev(labels), n_classes, value_max=VMAX,
                                     valid=None if valid is None else dev(valid))
    assert rows.dtype == torch.float32 and counts.dtype == torch.int64 and counts.device == rows.device
    return rows.cpu().numpy(), counts.cpu().numpy()


def check(rows, counts, cands, gt, labels, n_classes, valid=None, tag=""):
    """Both references, every class and candidate."""
    cands = [cands] if isinstance(cands, np.ndarray) else cands
    assert rows.shape == (len(cands), n_classes, 11) and counts.shape == (n_classes,)
    d_cands, d_gt = [dev(c) for c in cands], dev(gt)
    for k in range(n_classes):
        keep = labels == k if valid is None else (labels == k) & (valid != 0)
        assert counts[k] == keep.sum(), (tag, k, counts[k], keep.sum())
        loop, loop_n = S.scores_pooled(d_cands, d_gt, value_max=VMAX, valid=dev(keep))          # reference 2: the loop K22 replaces
        loop, loop_n = loop.cpu().numpy(), loop_n.cpu().numpy()
        assert loop_n[0] == counts[k]
        for c, cand in enumerate(cands):
            with np.errstate(all="ignore"):
                e = (cand - gt)[keep].astype(np.float32)
            if e.size == 0:
                assert np.isnan(rows[c, k]).all() and np.isnan(loop[c, 0]).all(), (tag, c, k, rows[c, k])
                continue
            assert rows[c, k, EXACT].tobytes() == loop[c, 0, EXACT].tobytes(), (tag, c, k, rows[c, k], loop[c, 0])
            R.check_row(rows[c, k], R.scores(e, VMAX), f"{tag} cand {c} class {k} n {e.size}")  # reference 1
            R.check_row(loop[c, 0], R.scores(e, VMAX), f"{tag} loop cand {c} class {k}")


def label_plane(kind, shape, n_classes, seed=0):
    n = int(np.prod(shape))
    rs = np.random.RandomState(seed + n_classes)
    if kind == "random":                   # every class, and 5 % that belong to none: 255, n_classes itself, 200
        lab = rs.randint(0, n_classes, n)
        none = rs.rand(n) < 0.05
        lab[none] = rs.choice([255, n_classes, 200], int(none.sum()))
    elif kind == "per_chunk":              # a whole run of 8192 pooled elements holds one class
        lab = (np.arange(n) // S.CHUNK) % n_classes
    elif kind == "hot99":                  # one class holds 99 %
        lab = np.zeros(n, dtype=np.int64)
        rest = rs.rand(n) >= 0.99
        lab[rest] = rs.randint(1, n_classes, int(rest.sum())) if n_classes > 1 else 255
    elif kind == "tiny":                   # class k holds exactly k elements, k < 4: the NaN row and the tiny counts
        lab = rs.randint(4, n_classes, n) if n_classes > 4 else np.full(n, 255)
        at = rs.permutation(n)[:6]
        for k, idx in ((1, at[:1]), (2, at[1:3]), (3, at[3:6])):
            if k < n_classes:
                lab[idx] = k
    else:
        raise KeyError(kind)
    return lab.astype(np.uint8).reshape(shape)


# ---- selection against both references -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "per_chunk", "hot99", "tiny", "random_valid50"])
@pytest.mark.parametrize("n_classes", [1, 3, 16, 32])
def test_chunk_boundaries(n_classes, kind):
    e = errors_case("chunks")                                                  # 25 500 elements: 3 runs of 8192 and one of 924
    assert e.size == 150 * 170 and (e.size + S.CHUNK - 1) // S.CHUNK == 4 and e.size % S.CHUNK == 924
    valid = None
    if kind == "random_valid50":
        kind, valid = "random", (np.random.RandomState(50).rand(*e.shape) < 0.5).astype(np.uint8)
    labels = label_plane(kind, e.shape, n_classes)
    rows, counts = by_class(e, np.zeros_like(e), labels, n_classes, valid)
    if kind == "tiny":
        assert counts[:4].tolist() == [0, 1, 2, 3][:n_classes]
    if kind == "hot99":
        assert counts[0] > 0.98 * e.size
    if kind == "random":
        assert ((labels >= n_classes).sum() > 0) and counts.sum() < e.size
    check(rows, counts, e, np.zeros_like(e), labels, n_classes, valid, tag=f"{kind} {n_classes}")


def test_one_class_of_zeros_is_the_masked_pooled_row():
    e = errors_case("chunks")
    valid = np.random.RandomState(51).rand(*e.shape) < 0.5
    labels = np.zeros(e.shape, np.uint8)
    rows, counts = by_class(e, np.zeros_like(e), labels, 1, valid.astype(np.uint8))
    want, n = S.scores_pooled(dev(e), dev(np.zeros_like(e)), value_max=VMAX, valid=dev(valid))
    want = want.cpu().numpy()
    assert counts.tolist() == n.cpu().tolist() == [int(valid.sum())]
    assert rows[0, 0, EXACT].tobytes() == want[0, 0, EXACT].tobytes()
    R.check_row(rows[0, 0], R.scores(e[valid], VMAX), "one class")
    plain, n_plain = by_class(e, np.zeros_like(e), labels, 1)                    # and without a plane: the unmasked pool
    assert n_plain.tolist() == [e.size]
    R.check_row(plain[0, 0], R.scores(e.reshape(-1), VMAX), "one class, no plane")


@pytest.mark.parametrize("name", ["quantised", "all_equal", "wide", "one_top_digit"])
def test_ties_and_digits(name):
    e = errors_case(name)
    labels = np.random.RandomState(41).randint(0, 3, e.shape).astype(np.uint8)
    rows, counts = by_class(e, np.zeros_like(e), labels, 3)
    check(rows, counts, e, np.zeros_like(e), labels, 3, tag=name)


def test_replicas():
    e = errors_case("replicated")                                              # 1.1e6 elements = 135 runs: 4 replicas
    labels = np.random.RandomState(4).choice(4, e.shape, p=[0.55, 0.3, 0.1, 0.05]).astype(np.uint8)
    rows, counts = by_class(e, np.zeros_like(e), labels, 4)
    check(rows, counts, e, np.zeros_like(e), labels, 4, tag="replicated")


def test_pitched_crops_of_two_scenes():
    """Two scenes of different shapes with a border crop (pitch != width), the prediction given in cropped form, 3 candidates."""
    rs = np.random.RandomState(9)
    shapes, b = [(70, 90), (64, 131)], 3
    gts = [rs.uniform(100, 600, s).astype(np.float32) for s in shapes]
    preds = [(g + rs.standard_normal(g.shape) * 1.5).astype(np.float32)[b:-b, b:-b] for g in gts]
    bases = [[(g + rs.standard_normal(g.shape) * s).astype(np.float32) for g in gts] for s in (4.0, 0.25)]
    labs = [rs.randint(0, 5, s).astype(np.uint8) for s in shapes]                 # label 4 >= n_classes: no class
    valids = [(rs.rand(*s) < 0.8).astype(np.uint8) for s in shapes]
    flat = lambda rasters: np.concatenate([np.ascontiguousarray(r).reshape(-1) for r in rasters])
    windows, off, p_off = [], 0, 0
    for (h, w) in shapes:
        ch, cw = h - 2 * b, w - 2 * b
        at = (off + b * w + b, w)
        windows.append((0, ch, cw, at, [(p_off, cw), at, at]))
        off, p_off = off + h * w, p_off + ch * cw
    cands = [dev(flat(preds)), dev(flat(bases[0])), dev(flat(bases[1]))]
    gt, labels, valid = dev(flat(gts)), dev(flat(labs)), dev(flat(valids))
    rows, counts = S.stratified_rows(cands, gt, windows, labels, 4, VMAX, valid=valid)
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    crop = lambda rasters: np.concatenate([r[b:-b, b:-b].reshape(-1) for r in rasters])
    cls = np.where(crop(valids) != 0, crop(labs), 255)
    e_all = [flat(preds) - crop(gts), crop(bases[0]) - crop(gts), crop(bases[1]) - crop(gts)]
    for k in range(4):
        assert counts[k] == (cls == k).sum() > 0
        keep = dev(((flat(labs) == k) & (flat(valids) != 0)).astype(np.uint8))
        loop, n = S.pooled_rows(cands, gt, windows, 1, VMAX, valid=keep)
        loop = loop.cpu().numpy()
        assert n.cpu().tolist() == [counts[k]]
        for c in range(3):
            assert rows[c, k, EXACT].tobytes() == loop[c, 0, EXACT].tobytes(), (c, k)
            R.check_row(rows[c, k], R.scores(e_all[c][cls == k].astype(np.float32), VMAX), f"pitched cand {c} class {k}")


# ---- what has no class has no influence ------------------------------------------------------------------------------
def poison_case():
    rs = np.random.RandomState(66)
    gt = rs.uniform(100, 600, (1, 97, 103)).astype(np.float32)                  # 9991 elements: two runs
    cands = [(gt + rs.standard_normal(gt.shape) * s).astype(np.float32) for s in (2.0, 0.5)]
    labels = rs.randint(0, 4, gt.shape).astype(np.uint8)
    labels[rs.rand(*gt.shape) < 0.15] = 255
    labels[rs.rand(*gt.shape) < 0.10] = 3                                        # >= n_classes = 3
    valid = (rs.rand(*gt.shape) < 0.7).astype(np.uint8)
    return gt, cands, labels, valid


def test_poison_at_ignored_and_masked_pixels_changes_no_byte():
    gt, cands, labels, valid = poison_case()
    none = (labels >= 3) | (valid == 0)
    assert ((labels == 255) & (valid != 0)).any() and ((labels == 3) & (valid != 0)).any() and ((labels < 3) & (valid == 0)).any()
    clean_c, clean_g = [np.where(none, 0, c).astype(np.float32) for c in cands], np.where(none, 0, gt).astype(np.float32)
    clean, clean_n = by_class(clean_c, clean_g, labels, 3, valid)
    poison = np.array([np.nan, np.inf, -np.inf, -32767.0, 1e30], dtype=np.float32)
    idx = np.flatnonzero(none.reshape(-1))
    for c in cands:
        c.reshape(-1)[idx] = poison[np.arange(idx.size) % 5]
    gt.reshape(-1)[idx] = poison[(np.arange(idx.size) // 5) % 5]                # every pair of poisons meets
    rows, counts = by_class(cands, gt, labels, 3, valid)
    assert np.isfinite(rows).all()
    assert rows.tobytes() == clean.tobytes() and counts.tolist() == clean_n.tolist()
    check(rows, counts, cands, gt, labels, 3, valid, tag="poison")


def test_one_counted_nan_touches_one_row():
    gt, cands, labels, valid = poison_case()
    before, n_before = by_class(cands, gt, labels, 3, valid)
    at = np.flatnonzero(((labels == 1) & (valid != 0)).reshape(-1))[321]
    cands[0].reshape(-1)[at] = np.nan
    rows, counts = by_class(cands, gt, labels, 3, valid)
    assert np.isnan(rows[0, 1, :5]).all() and np.isfinite(rows[0, 1, 5:]).all()
    assert counts.tolist() == n_before.tolist()
    for c in range(2):
        for k in range(3):
            if (c, k) != (0, 1):
                assert rows[c, k].tobytes() == before[c, k].tobytes(), (c, k)


def test_rows_do_not_depend_on_the_rest_of_the_call():
    gt, cands, labels, valid = poison_case()
    rs = np.random.RandomState(8)
    eight = cands + [(gt + rs.standard_normal(gt.shape) * s).astype(np.float32) for s in (0.1, 1.0, 3.0, 9.0, 27.0, 81.0)]
    full, full_n = by_class(eight, gt, labels, 3, valid)
    again, again_n = by_class(eight, gt, labels, 3, valid)                       # two runs
    assert again.tobytes() == full.tobytes() and again_n.tolist() == full_n.tolist()
    for c in (0, 5, 7):                                                          # 1 candidate or 8
        one, one_n = by_class(eight[c], gt, labels, 3, valid)
        assert one.tobytes() == full[c:c + 1].tobytes() and one_n.tolist() == full_n.tolist(), c
    other = [c.copy() for c in eight]                                            # new values at class 1's pixels
    g2 = gt.copy()
    for a in other + [g2]:
        a[labels == 1] = rs.uniform(-1e4, 1e4, int((labels == 1).sum())).astype(np.float32)
    moved, moved_n = by_class(other, g2, labels, 3, valid)
    assert moved[:, 0].tobytes() == full[:, 0].tobytes() and moved[:, 2].tobytes() == full[:, 2].tobytes()
    assert moved[:, 1].tobytes() != full[:, 1].tobytes() and moved_n.tolist() == full_n.tolist()
    more, more_n = by_class(eight, gt, labels, 4, valid)                         # one more class in the call: label 3 now counts
    assert more[:, :3].tobytes() == full.tobytes() and more_n[:3].tolist() == full_n.tolist() and more_n[3] > 0


def test_the_number_of_launches_does_not_depend_on_n_classes():
    e = errors_case("chunks")
    per = []
    for n_classes, n_cand in ((1, 1), (32, 1), (3, 8)):
        labels = label_plane("random", e.shape, n_classes)
        prepares, before = launches(CENSUS[0]), launches(*CENSUS)
        by_class([e] * n_cand, np.zeros_like(e), labels, n_classes)
        per.append(launches(*CENSUS) - before)
        assert launches(CENSUS[0]) == prepares + 1
    assert per == [16, 16, 16]


# ---- summarise_by_class ----------------------------------------------------------------------------------------------
def small_store():
    rs = np.random.RandomState(23)
    shapes = [(48, 60), (40, 52)]
    gts = [rs.uniform(150, 400, s).astype(np.float32) + 37 * i for i, s in enumerate(shapes)]
    lrs = [g + rs.uniform(-5, 5, g.shape).astype(np.float32) for g in gts]
    scenes = D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, elev_min=-80,
                            elev_max=933, elev_log=True, device=DEV)
    other = [g + rs.standard_normal(g.shape).astype(np.float32) * 8 for g in gts]
    preds = [(g + rs.standard_normal(g.shape) * 1.5).astype(np.float32) for g in gts]
    return scenes, gts, lrs, other, preds, rs


def test_summarise_by_class_against_the_loop_over_summarise():
    scenes, gts, lrs, other, preds, rs = small_store()
    b = 1                                                                        # int(32 * 0.05)
    names = ["water", "forest", "built", "empty"]
    labs = [rs.choice([0, 1, 2, 255], g.shape, p=[0.2, 0.5, 0.2, 0.1]).astype(np.uint8) for g in gts]
    valids = [rs.rand(*g.shape) < 0.8 for g in gts]
    given = [preds[0][b:-b, b:-b].copy(), preds[1]]                               # a cropped and a whole raster
    kw = dict(baselines={"COP30": "lr_dem", "other": other}, value_max=VMAX, border=0.05, patch_size=32)
    before = launches(*CENSUS)
    table = S.summarise_by_class(scenes, given, labs, names, valid=valids, **kw)
    assert launches(*CENSUS) == before + 16
    flat = dev(np.concatenate([l.reshape(-1) for l in labs]))
    assert _nan_to_none(S.summarise_by_class(scenes, given, flat, names, valid=valids, **kw)) == _nan_to_none(table)
    assert list(table) == ["SR", "COP30", "other"]
    cls = np.concatenate([np.where(R.crop(v, b, v.shape) != 0, R.crop(l, b, l.shape), 255) for v, l in zip(valids, labs)]).astype(np.int64)
    for k, cname in enumerate(names):
        loop = S.summarise(scenes, given, valid=[v & (l == k) for v, l in zip(valids, labs)], **kw)
        for name, rasters in (("SR", preds), ("COP30", lrs), ("other", other)):
            got, ek = table[name][cname], R.errors(rasters, gts, b)[cls == k]
            assert got["N"] == loop[name]["N"] == ek.size
            if ek.size == 0:
                assert cname == "empty" and all(np.isnan(got[c]) and np.isnan(loop[name][c]) for c in R.COLUMNS)
                continue
            assert got["Median"] == loop[name]["Median"]
            want = R.scores(ek, VMAX)
            R.check_row(np.array([got[c] for c in R.COLUMNS] + list(want["brackets"])), want, f"{name} {cname}")
            R.check_row(np.array([loop[name][c] for c in R.COLUMNS] + list(want["brackets"])), want, f"loop {name} {cname}")
    for name in table:
        assert abs(sum(t["share"] for t in table[name].values()) - 1.0) < 1e-12
        assert sum(t["N"] for t in table[name].values()) == int((cls < 4).sum())


def _nan_to_none(tree):
    if isinstance(tree, dict):
        return {k: _nan_to_none(v) for k, v in tree.items()}
    return None if isinstance(tree, float) and tree != tree else tree


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    before = launches(*CENSUS, b"slope_classes")
    gt = torch.zeros(64, device=DEV)
    win = [(0, 8, 8, (0, 8), [(0, 8)])]
    ok = torch.zeros(64, dtype=torch.uint8, device=DEV)
    for bad in (ok.float(), ok.bool(), ok[:63], torch.zeros(65, dtype=torch.uint8, device=DEV), ok.cpu(), ok.view(8, 8)):
        with pytest.raises(ValueError, match="labels"):
            S.stratified_rows([gt], gt, win, bad, 2, VMAX)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="n_classes"):
            S.stratified_rows([gt], gt, win, ok, bad, VMAX)
        with pytest.raises(ValueError, match="n_classes"):
            S.scores_by_class(gt.view(8, 8), gt.view(8, 8), ok.view(8, 8), bad)
    scenes, gts, lrs, other, preds, rs = small_store()
    kw = dict(value_max=VMAX, border=0.05, patch_size=32)
    cropped = sum((h - 2) * (w - 2) for h, w in scenes.shapes)
    for bad in (torch.zeros(cropped, dtype=torch.uint8, device=DEV),              # the cropped layout instead of the store's
                torch.zeros(48 * 60 + 40 * 52, dtype=torch.uint8), torch.zeros(48 * 60 + 40 * 52, dtype=torch.int32, device=DEV),
                [np.zeros((46, 58), np.uint8), np.zeros((38, 50), np.uint8)]):
        with pytest.raises(ValueError, match="labels"):
            S.summarise_by_class(scenes, preds, bad, ["a", "b"], **kw)
    with pytest.raises(ValueError, match="class names"):
        S.summarise_by_class(scenes, preds, [np.zeros(s, np.uint8) for s in scenes.shapes], [str(i) for i in range(33)], **kw)
    with pytest.raises(ValueError, match="slope_thresholds"):
        S.slope_class_plane(scenes, [15.0, 5.0], 1.0)
    assert launches(*CENSUS, b"slope_classes") == before
