"""K21 on the MI355X: the float16 histogram of the pooled errors (jspsr_errdist_hist_forward) and the Gaussian KDE evaluated
from it (jspsr_errdist_kde_forward) against the restatement built from the raw errors (tests/errdist_ref.py: numpy filter,
astype(float16), np.unique; the curve as a direct fp64 sum over all n points).

Histograms and counts are compared with integer equality.  The curve's tolerances are `errdist_ref.check_curve`'s: support
rtol 1e-12, density rtol 1e-9 plus atol 1e-12 x the peak (both sides fp64; derivation there)."""
import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import summary as S
from tests import errdist_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def launches(*names):
    return sum(_lib.load().jspsr_launch_count(n) for n in names)


def one_window(n, n_cand=1):
    return [(0, 1, n, (0, n), [(0, n)] * n_cand)]


def device_hist(cands, gt, wins, lo=-5.0, hi=5.0, valid=None):
    """numpy flat buffers -> (hist, counts) as numpy, key0."""
    hist, counts, key0 = S.pooled_histogram([torch.from_numpy(c).to(DEV) for c in cands], torch.from_numpy(gt).to(DEV), wins, lo, hi,
                                            valid=None if valid is None else torch.from_numpy(valid).to(DEV))
    assert hist.dtype == torch.int64 and counts.dtype == torch.int64 and hist.device == counts.device and hist.is_cuda
    assert hist.shape == (len(cands), R.bins(lo, hi)[1]) and counts.shape == (len(cands), 4)
    return hist.cpu().numpy(), counts.cpu().numpy(), key0


def gather(a, wins, which=None):
    out = []
    for _, h, w, g_, cs in wins:
        off, pitch = g_ if which is None else cs[which]
        out.append(a[off + np.arange(h)[:, None] * pitch + np.arange(w)[None, :]].reshape(-1))
    return np.concatenate(out)


def check_hist(hist, counts, key0, cands, gt, wins, lo=-5.0, hi=5.0, valid=None, tag=""):
    keep = slice(None) if valid is None else gather(valid, wins) != 0
    for c, cand in enumerate(cands):
        with np.errstate(invalid="ignore", over="ignore"):
            e = (gather(cand, wins, c) - gather(gt, wins)).astype(np.float32)[keep]
        h, n, k0 = R.histogram(e, lo, hi)
        assert k0 == key0 and tuple(counts[c].tolist()) == n, (tag, c, counts[c], n)
        bad = np.nonzero(hist[c] != h)[0]
        assert bad.size == 0, (tag, c, [(int(b), int(hist[c][b]), int(h[b])) for b in bad[:5]])
        assert hist[c].sum() == n[1]


# ---- the rounding on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(-65504.0, 65504.0), (-5.0, 5.0)])
def test_designed_operands(lo, hi):
    x = np.concatenate([R.exhaustive_values(), np.array([np.nan, np.inf, -np.inf], dtype=np.float32)])
    gt = np.zeros_like(x)
    before = launches(b"errdist_hist")
    hist, counts, key0 = device_hist([x], gt, one_window(x.size), lo, hi)
    assert launches(b"errdist_hist") == before + 1                               # one launch, also for two LDS images
    check_hist(hist, counts, key0, [x], gt, one_window(x.size), lo, hi, tag="gt = 0")
    assert counts[0, 0] - counts[0, 1:].sum() == 1                               # the NaN
    if hi > 60000:
        assert (hist[0] > 0).sum() == 63488                                      # every finite float16 value was produced
    # the same list spread over both rasters so that the subtraction is exact: x = a - b with a the upper bits of x
    f = x[np.isfinite(x)]
    a = (f.view(np.uint32) & np.uint32(0xfffff000)).view(np.float32)
    b = a - f                                                                    # f == a: +0, and a - (+0) keeps the sign of a -0
    assert ((a - b).view(np.uint32) == f.view(np.uint32)).all() and (b != 0).sum() > 100000
    hist2, counts2, _ = device_hist([a], b, one_window(f.size), lo, hi)
    check_hist(hist2, counts2, key0, [a], b, one_window(f.size), lo, hi, tag="spread")
    h, n, _ = R.histogram(f, lo, hi)
    assert np.array_equal(hist2[0], h)


# ---- the pooled walk -------------------------------------------------------------------------------------------------
def walk_case():
    rs = np.random.RandomState(7)
    shapes, b = [(37, 53), (64, 64), (129, 40)], 3
    gts = [rs.uniform(100, 600, s).astype(np.float32) for s in shapes]
    base = [[(g + rs.standard_normal(g.shape) * sd).astype(np.float32) for g in gts] for sd in (2.5, 6.0)]
    pred = [(g + rs.standard_normal(g.shape) * 0.7).astype(np.float32)[b:-b, b:-b] for g in gts]      # cropped: another pitch
    gt = np.concatenate([g.reshape(-1) for g in gts])
    cands = [np.concatenate([p.reshape(-1) for p in pred])] + [np.concatenate([r.reshape(-1) for r in rr]) for rr in base]
    wins, off, poff = [], 0, 0
    for i, (h, w) in enumerate(shapes):
        ch, cw = h - 2 * b, w - 2 * b
        at = (off + b * w + b, w)
        wins.append((i, ch, cw, at, [(poff, cw), at, at]))                        # the segment entry is not read
        off += h * w
        poff += ch * cw
    col = (37 * 53 + 5 * 64 + 9, 64)                                              # a window of width 1: a column of scene 1
    wins.insert(1, (0, 40, 1, col, [(31 * 47 + 2 * 58 + 6, 58), col, col]))
    return gt, cands, wins


def test_pooled_walk_over_pitched_windows():
    gt, cands, wins = walk_case()
    total = sum(w[1] * w[2] for w in wins)
    assert total > 8192 and total % 8192 and total % 4096                         # several workgroups, a partly filled last step
    hist, counts, key0 = device_hist(cands, gt, wins)
    check_hist(hist, counts, key0, cands, gt, wins, tag="walk")
    assert (counts[:, 0] == total).all() and counts[2, 2] > 0 and counts[2, 3] > 0
    # more elements than workgroups times one step: every workgroup loops, windows straddle the ranges
    rs = np.random.RandomState(8)
    big = rs.uniform(0, 50, 1500 * 1100).astype(np.float32)
    c2 = (big + rs.standard_normal(big.size) * 3).astype(np.float32)
    w2 = [(0, 701, 997, (3 * 1100 + 5, 1100), [(7, 1100)]), (0, 650, 1, (11, 1100), [(900 * 1100, 1)]), (0, 333, 1100, (0, 1100), [(1100, 1100)])]
    assert sum(w[1] * w[2] for w in w2) > 256 * 4096
    hist, counts, key0 = device_hist([c2], big, w2)
    check_hist(hist, counts, key0, [c2], big, w2, tag="big")


# ---- the mask --------------------------------------------------------------------------------------------------------
def test_masked_elements_influence_nothing():
    gt, cands, wins = walk_case()
    rs = np.random.RandomState(9)
    valid = (rs.rand(gt.size) < 0.6).astype(np.uint8) * 5                        # any non-zero byte keeps
    clean_hist, clean_counts, key0 = device_hist(cands, gt, wins, valid=valid)
    poison = np.array([np.nan, np.inf, -np.inf, -32767.0, 1e30], dtype=np.float32)
    gt2, cands2 = gt.copy(), [c.copy() for c in cands]
    hole = np.nonzero(valid == 0)[0]
    gt2[hole] = poison[np.arange(hole.size) % 5]
    for k, c in enumerate(cands2[1:]):                                            # the baselines share gt's layout
        c[hole] = poison[(np.arange(hole.size) + k + 1) % 5]
    for _, h, w, (go, gp), cs in wins:                                            # the prediction has its own layout: poisoned through the windows
        rows, cols = np.arange(h)[:, None], np.arange(w)[None, :]
        m = valid[go + rows * gp + cols] == 0
        idx = (cs[0][0] + rows * cs[0][1] + cols)[m]
        cands2[0][idx] = poison[idx % 5]
    before = launches(b"errdist_hist (valid)")
    hist, counts, _ = device_hist(cands2, gt2, wins, valid=valid)
    assert launches(b"errdist_hist (valid)") == before + 1
    assert np.array_equal(hist, clean_hist) and np.array_equal(counts, clean_counts)
    check_hist(hist, counts, key0, cands2, gt2, wins, valid=valid, tag="speckled")
    assert 0 < counts[0, 0] < sum(w[1] * w[2] for w in wins) and (counts[:, 0] - counts[:, 1:].sum(axis=1) == 0).all()
    plain = device_hist(cands, gt, wins)
    ones = device_hist(cands, gt, wins, valid=np.ones(gt.size, np.uint8))
    assert np.array_equal(plain[0], ones[0]) and np.array_equal(plain[1], ones[1])
    zh, zc, _ = device_hist(cands2, gt2, wins, valid=np.zeros(gt.size, np.uint8))
    assert not zh.any() and not zc.any()
    support, density, stats = S.kde_curves(torch.from_numpy(zh).to(DEV), key0)
    assert torch.isnan(support).all() and torch.isnan(density).all() and torch.isnan(stats).all()


# ---- hot bins --------------------------------------------------------------------------------------------------------
def test_hot_bins_count_exactly():
    n = 512 * 300                                                                 # 153 600 > 2^17: a 16-bit counter anywhere overflows
    rs = np.random.RandomState(10)
    gt = np.zeros(n, np.float32)
    same = np.full(n, 0.375, np.float32)
    two = np.where(rs.rand(n) < 0.3, np.float32(-1.25), np.float32(2.5)).astype(np.float32)
    zeros = np.zeros(n, np.float32)
    zeros[rs.choice(n, 11, replace=False)] = -0.0
    half = np.where(rs.rand(n) < 0.5, np.float32(0), rs.standard_normal(n).astype(np.float32)).astype(np.float32)
    cands = [same, two, zeros, half]
    wins = [(0, 512, 300, (0, 300), [(0, 300)] * 4)]
    hist, counts, key0 = device_hist(cands, gt, wins)
    check_hist(hist, counts, key0, cands, gt, wins, tag="hot")
    zero = 0x8000 - key0
    assert hist[0].max() == n and (hist[0] > 0).sum() == 1
    assert sorted(hist[1][hist[1] > 0].tolist()) == sorted([int((two < 0).sum()), int((two > 0).sum())])
    assert hist[2][zero] == n - 11 and hist[2][zero - 1] == 11
    assert hist[3][zero] > n // 2 - 2000


# ---- a range of more bins than one LDS image -------------------------------------------------------------------------
def test_wide_range_is_exact():
    rs = np.random.RandomState(11)
    n = 300000
    gt = rs.uniform(0, 900, n).astype(np.float32)
    cands = [(gt + rs.standard_normal(n) * sd).astype(np.float32) for sd in (40.0, 3.0)]
    cands[0][:7] = gt[:7] + np.array([100.0, -100.0, 99.97, -99.97, 100.5, -100.5, 0.0], dtype=np.float32)
    assert R.bins(-100, 100)[1] == 44162
    hist, counts, key0 = device_hist(cands, gt, one_window(n, 2), -100.0, 100.0)
    check_hist(hist, counts, key0, cands, gt, one_window(n, 2), -100.0, 100.0, tag="wide")
    assert hist[0][:100].sum() > 0 and hist[0][-100:].sum() > 0 and counts[0, 2] > 0 and counts[0, 3] > 0
    assert hist[0][36864:].sum() > 1000                                           # the second image was filled


# ---- independence ----------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_call_or_the_run():
    rs = np.random.RandomState(12)
    n = 70001
    gt = rs.uniform(0, 100, n).astype(np.float32)
    cands = [(gt + rs.standard_normal(n) * (0.2 + 0.9 * k) + 0.3 * k).astype(np.float32) for k in range(8)]
    cands[5] = gt.copy()
    hist, counts, key0 = device_hist(cands, gt, one_window(n, 8))
    check_hist(hist, counts, key0, cands, gt, one_window(n, 8), tag="eight")
    for k in range(8):
        h1, c1, _ = device_hist([cands[k]], gt, one_window(n, 1))
        assert np.array_equal(h1[0], hist[k]) and np.array_equal(c1[0], counts[k]), k
    again = device_hist(cands, gt, one_window(n, 8))
    assert again[0].tobytes() == hist.tobytes() and again[1].tobytes() == counts.tobytes()
    h_dev = torch.from_numpy(hist).to(DEV)
    before = launches(b"errdist_kde")
    first = [t.cpu().numpy() for t in S.kde_curves(h_dev, key0)]
    assert launches(b"errdist_kde") == before + 2
    second = [t.cpu().numpy() for t in S.kde_curves(h_dev, key0)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    alone = [t.cpu().numpy() for t in S.kde_curves(h_dev[3], key0)]
    assert all(a.tobytes() == b[3].tobytes() for a, b in zip(alone, first))
    assert np.isnan(first[1][5]).all() and np.isfinite(first[1][[0, 1, 2, 3, 4, 6, 7]]).all()      # no variance: every error is 0


# ---- the curve -------------------------------------------------------------------------------------------------------
def error_shapes(name):
    rs = np.random.RandomState(len(name))
    n = 100000
    if name == "normal":
        return (rs.standard_normal(n) * 1.3 + 0.2).astype(np.float32)
    if name == "bimodal":
        return np.where(rs.rand(n) < 0.35, rs.standard_normal(n) * 0.4 - 2.0, rs.standard_normal(n) * 0.9 + 1.5).astype(np.float32)
    return (rs.standard_normal(n) * 9.0 + 3.0).astype(np.float32)                 # heavily clipped: most of it is outside [-5, 5]


@pytest.mark.parametrize("name", ["normal", "bimodal", "clipped"])
@pytest.mark.parametrize("kw", [dict(), dict(gridsize=97, cut=0.0, bw_adjust=0.5)])
def test_curve_against_the_restatement(name, kw):
    e = error_shapes(name)
    gt = np.zeros_like(e)
    hist, counts, key0 = S.pooled_histogram([torch.from_numpy(e).to(DEV)], torch.from_numpy(gt).to(DEV), one_window(e.size))
    support, density, stats = S.kde_curves(hist, key0, **kw)
    assert support.dtype == density.dtype == stats.dtype == torch.float64 and support.is_cuda
    x = R.clipped(e)
    assert counts[0, 1].item() == x.size and (name != "clipped" or x.size < 0.5 * e.size)
    want_s, want_d, want_st = R.curve(x, **kw)
    R.check_curve(support[0].cpu().numpy(), density[0].cpu().numpy(), want_s, want_d, name)
    assert np.allclose(stats[0].cpu().numpy(), want_st, rtol=1e-12, atol=0)
    hs, hd, hst = S.kde_curves(hist.cpu(), key0, **kw)                            # the host path, same formulas
    R.check_curve(hs[0].numpy(), hd[0].numpy(), want_s, want_d, name + " host")


def test_degenerate_curves_are_nan():
    key0, K = S.histogram_bins()
    h = torch.zeros((4, K), dtype=torch.int64)
    h[1, 100] = 1                                                                 # n_in = 1
    h[2, 200] = 50                                                                # no variance
    h[3, 300], h[3, 30000] = 2, 3
    support, density, stats = (t.cpu() for t in S.kde_curves(h.to(DEV), key0))
    v = S.histogram_values(key0, K)
    assert torch.isnan(support[:3]).all() and torch.isnan(density[:3]).all()
    assert torch.isfinite(support[3]).all() and torch.isfinite(density[3]).all()
    assert torch.isnan(stats[0]).all() and stats[1, 0] == v[100] and torch.isnan(stats[1, 1:]).all()
    assert stats[2].tolist() == [float(v[200]), 0.0, 0.0]
    x = np.array([v[300]] * 2 + [v[30000]] * 3)
    want_s, want_d, _ = R.curve(x)
    R.check_curve(support[3].numpy(), density[3].numpy(), want_s, want_d, "five points")


# ---- error_distribution ----------------------------------------------------------------------------------------------
def by_hand(rasters, gts, valids, b, lo, hi, **kw):
    crop = lambda a: a[b:a.shape[0] - b, b:a.shape[1] - b] if a.shape == gts[0].shape else a
    with np.errstate(invalid="ignore"):
        e = np.concatenate([(crop(r) - crop(g))[crop(v)] for r, g, v in zip(rasters, gts, valids)]).astype(np.float32)
    hist, n, key0 = R.histogram(e, lo, hi)
    return R.curve(R.clipped(e, lo, hi), **kw), n


@pytest.mark.parametrize("form", ["collector", "rasters"])
@pytest.mark.parametrize("with_valid", [False, True])
def test_error_distribution_against_the_route_by_hand(form, with_valid):
    full, k, n, border = 70, 32, 9, 0.05
    rs = np.random.RandomState(13)
    gts = [rs.uniform(150, 400, (full, full)).astype(np.float32) + 37 * i for i in range(3)]
    lrs = [g + rs.uniform(-7, 7, g.shape).astype(np.float32) for g in gts]
    other = [g + (rs.standard_normal(g.shape) * 2).astype(np.float32) for g in gts]
    scenes = D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, elev_min=-80,
                            elev_max=933, elev_log=True, device=DEV)
    b = int(k * border)
    valids = [rs.rand(full, full) < 0.7 if with_valid else np.ones((full, full), bool) for _ in gts]
    if form == "collector":
        lo, hi = -400.0, 400.0                                                    # random tiles: errors of hundreds of metres
        c = S.ScenePredictions(scenes, k, n, border=border)
        c.add(torch.from_numpy(rs.uniform(0.55, 0.8, (3 * n, 1, k, k)).astype(np.float32)).to(DEV))
        preds = [c.rasters()[sid] for sid in scenes.ids]                          # cropped mosaics
        given = c
    else:
        lo, hi = -5.0, 5.0
        preds = [(g + rs.standard_normal(g.shape) * 2.5).astype(np.float32) for g in gts]
        for p, v in zip(preds, valids):
            p[~v] = -32767.0
        given = [preds[0], preds[1][b:-b, b:-b].copy(), torch.from_numpy(preds[2])]
    kw = dict(gridsize=50, cut=0.5, bw_adjust=1.0)
    got = S.error_distribution(scenes, given, baselines={"COP30": "lr_dem", "other": other}, border=border, patch_size=k,
                               valid=valids if with_valid else None, lo=lo, hi=hi, **kw)
    assert list(got) == ["SR", "COP30", "other"]
    for name, rasters in (("SR", preds), ("COP30", lrs), ("other", other)):
        (support, dens, (mean, sd, bw)), cnt = by_hand(rasters, gts, valids, b, lo, hi, **kw)
        g = got[name]
        assert (g["n"], g["n_in"], g["n_below"], g["n_above"]) == cnt and cnt[1] > 1000, (name, cnt)
        R.check_curve(g["support"], g["density"], support, dens, name)
        assert np.allclose([g["mean"], g["std"], g["bw"]], [mean, sd, bw], rtol=1e-12, atol=0)
    assert got["COP30"]["n_below"] + got["COP30"]["n_above"] > 0 or form == "collector"
