"""The error distribution (K21) without a GPU: the host twins of the kernel's float16 rounding and classification
(`jspsr_errdist_key`, `jspsr_errdist_bins`) against `np.float32(x).astype(np.float16)` on every finite float16 value, each
value's upper halfway point in fp32 and that point's two fp32 neighbours; the restatement's curve (tests/errdist_ref.py, a
direct sum over the raw points) against scipy.stats.gaussian_kde; the host paths of `pooled_histogram`, `histogram_values`,
`kde_curves` and `error_distribution` against the restatement; argument errors in Python and at the C entries before any
launch; header, binding and library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import summary as S
from tests import errdist_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"jspsr_errdist_bins": 4, "jspsr_errdist_key": 3, "jspsr_errdist_workspace_bytes": 2, "jspsr_errdist_hist_forward": 15,
           "jspsr_errdist_kde_forward": 12}
P = dict(elev_min=-80, elev_max=933, elev_log=True)


# ---- the host twins --------------------------------------------------------------------------------------------------
def want_keys(x, lo, hi):
    """numpy's classification: the bin, or -1 below, -2 above, -3 NaN."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    key0, K = R.bins(lo, hi)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (x >= lo32) & (x <= hi32)
        want = np.where(x < lo32, -1, np.where(x > hi32, -2, -3)).astype(np.int64)
        want[inside] = np.clip(R.f16_key(x[inside].astype(np.float16).view(np.uint16)) - key0, 0, K - 1)
    return want


@pytest.mark.parametrize("lo,hi", [(-65504.0, 65504.0), (-5.0, 5.0), (-100.0, 100.0), (0.0, 1.0), (-2.0 ** -20, 2.0 ** -20)])
def test_host_twin_rounds_as_numpy_astype(lo, hi):
    lib = _lib.load()
    x = np.concatenate([R.exhaustive_values(), np.array([np.nan, np.inf, -np.inf], dtype=np.float32)])
    assert x.size > 4 * 63000
    want = want_keys(x, lo, hi)
    key = lib.jspsr_errdist_key
    got = np.array([key(float(v), lo, hi) for v in x], dtype=np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(x[i], got[i], want[i]) for i in bad[:5]]
    if (lo, hi) == (-65504.0, 65504.0):                                          # every rounding decision was in range
        assert (want >= 0).sum() >= 4 * 63000 and want.max() == 63487 and want.min() == -3


def test_named_operands():
    lib = _lib.load()
    key0, K = ctypes.c_int(), ctypes.c_int()
    assert lib.jspsr_errdist_bins(-5.0, 5.0, ctypes.byref(key0), ctypes.byref(K)) == 0
    assert (key0.value, K.value) == R.bins(-5, 5) == S.histogram_bins(-5, 5) and K.value == 35330
    assert key0.value == (0xc500 ^ 0xffff) and key0.value + K.value - 1 == (0x4500 ^ 0x8000)
    k0w, Kw = ctypes.c_int(), ctypes.c_int()
    assert lib.jspsr_errdist_bins(-100.0, 100.0, ctypes.byref(k0w), ctypes.byref(Kw)) == 0 and Kw.value == 44162
    assert S.histogram_bins(-100, 100)[1] == 44162

    def key(e):
        return lib.jspsr_errdist_key(float(np.float32(e)), -5.0, 5.0)

    zero = 0x8000 - key0.value
    assert key(0.0) == zero and key(-0.0) == zero - 1                            # two neighbouring bins of value 0
    assert key(5.0) == K.value - 1 and key(-5.0) == 0
    assert key(4.999) == K.value - 1 and key(-4.999) == 0                        # in range, rounds to +-5.0
    assert key(np.nextafter(np.float32(5), np.float32(9))) == -2 and key(np.nextafter(np.float32(-5), np.float32(-9))) == -1
    assert key(np.inf) == -2 and key(-np.inf) == -1 and key(np.nan) == -3
    assert key(2.0 ** -24) == zero + 1 and key(2.0 ** -25) == zero               # the smallest subnormal; the tie below it goes to even
    assert key(np.nextafter(np.float32(2.0 ** -25), np.float32(1))) == zero + 1 and key(-2.0 ** -24) == zero - 2
    assert key(1e-30) == zero and key(-1e-30) == zero - 1
    assert lib.jspsr_errdist_key(-0.0, 0.0, 1.0) == 0                            # lo = +0 keeps -0, counted with +0
    vals = S.histogram_values(key0.value, K.value).numpy()
    assert vals.dtype == np.float64 and vals.shape == (35330,)
    assert vals[0] == -5.0 and vals[-1] == 5.0 and vals[zero] == 0.0 and vals[zero - 1] == 0.0 and np.signbit(vals[zero - 1])
    assert np.all(np.diff(vals) >= 0) and (np.diff(vals) == 0).sum() == 1
    for lo, hi in ((1.0, 0.0), (np.nan, 1.0), (0.0, np.inf), (-70000.0, 0.0), (0.0, 65504.1)):
        assert lib.jspsr_errdist_bins(lo, hi, ctypes.byref(key0), ctypes.byref(K)) == -1 and b"errdist_bins" in lib.jspsr_last_error()
        assert lib.jspsr_errdist_key(0.5, lo, hi) == -4
        with pytest.raises(ValueError, match="histogram_bins"):
            S.histogram_bins(lo, hi)
    assert lib.jspsr_errdist_bins(-5.0, 5.0, None, ctypes.byref(K)) == -1


# ---- the restatement against scipy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bw_adjust", [1.0, 0.5])
def test_restatement_is_scipys_gaussian_kde(bw_adjust):
    stats = pytest.importorskip("scipy.stats")
    rs = np.random.RandomState(21)
    x = R.clipped(rs.standard_normal(20000) * 1.3 + 0.2)
    support, dens, (mean, sd, bw) = R.curve(x, 200, 0.5, bw_adjust)
    kde = stats.gaussian_kde(x)                                                   # what seaborn 0.12+ does: scott, then the adjustment
    kde.set_bandwidth(kde.factor * bw_adjust)
    assert abs(np.sqrt(kde.covariance.squeeze()) - bw) <= 1e-13 * bw
    want = kde(support)
    assert np.all(np.abs(dens - want) <= 1e-10 * want.max())
    assert support[0] == x.min() - 0.5 * bw and support[-1] == x.max() + 0.5 * bw and support.shape == (200,)
    # ... and the sum over distinct values weighted by their counts is the sum over the points
    hist, counts, key0 = R.histogram(x.astype(np.float32))
    s2, d2, st2 = (t.numpy() for t in S.kde_curves(torch.from_numpy(hist), key0, 200, 0.5, bw_adjust))
    R.check_curve(s2, d2, support, dens, "host kde")
    assert np.allclose(st2, [mean, sd, bw], rtol=1e-12, atol=0)


# ---- host paths ------------------------------------------------------------------------------------------------------
def pool_case():
    rs = np.random.RandomState(5)
    gt = rs.uniform(100, 600, 2000).astype(np.float32)
    cands = [(gt + rs.standard_normal(gt.shape) * s).astype(np.float32) for s in (0.8, 4.0)]
    cands.append(gt.copy())
    valid = (rs.rand(gt.size) < 0.7)
    for c in cands[:2]:
        c[~valid] = -32767.0
        c[7], c[8] = np.nan, np.inf
    gt[~valid & (np.arange(gt.size) % 3 == 0)] = np.nan
    valid[7] = valid[8] = True
    gt[7] = gt[8] = 300.0
    # windows over a 40-wide raster of 50 rows: (segment, h, w, gt at, cands at); the segment entry is not read
    wins = [(3, 10, 17, (3, 40), [(3, 40)] * 3), (0, 5, 1, (1200, 40), [(1200, 40)] * 3), (9, 12, 40, (1520, 40), [(1520, 40)] * 3)]
    return gt, cands, valid, wins


def gather(a, wins, which=None):
    out = []
    for _, h, w, g_, cs in wins:
        off, pitch = g_ if which is None else cs[which]
        out.append(a[off + np.arange(h)[:, None] * pitch + np.arange(w)[None, :]].reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize("masked", [False, True])
def test_pooled_histogram_host_path(masked):
    gt, cands, valid, wins = pool_case()
    if not masked:
        gt = np.nan_to_num(gt, nan=250.0)
    cands[2] = gt.copy()                                                         # the hot bin: every scored error is +0
    v = torch.from_numpy(valid.astype(np.uint8) * 3) if masked else None
    hist, counts, key0 = S.pooled_histogram([torch.from_numpy(c) for c in cands], torch.from_numpy(gt), wins, valid=v)
    assert hist.dtype == torch.int64 and hist.shape == (3, 35330) and counts.shape == (3, 4) and key0 == R.bins(-5, 5)[0]
    keep = gather(valid, wins) if masked else slice(None)
    for c, cand in enumerate(cands):
        with np.errstate(invalid="ignore"):
            e = (gather(cand, wins, c) - gather(gt, wins))[keep]
        h, n, k0 = R.histogram(e)
        assert np.array_equal(hist[c].numpy(), h) and tuple(counts[c].tolist()) == n and k0 == key0, c
        assert n[0] - sum(n[1:]) == int(np.isnan(e).sum())
    assert counts[0, 0] == counts[1, 0] == counts[2, 0]
    assert hist[2].sum() == hist[2, 0x8000 - key0] == counts[2, 1]                # everything in the bin of +0
    if not masked:
        assert counts[0, 3] >= 1 and counts[0, 0] - counts[0, 1:].sum() == 1       # the inf above, the NaN nowhere


def cpu_scenes(n_sc=3, full=20, seed=5):
    rs = np.random.RandomState(seed)
    gts = [rs.uniform(150, 400, (full, full)).astype(np.float32) + 37 * i for i in range(n_sc)]
    lrs = [g + rs.uniform(-7, 7, g.shape).astype(np.float32) for g in gts]
    scenes = D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, device="cpu", **P)
    return scenes, gts, lrs, rs


def by_hand(rasters, gts, valids, b, **kw):
    crop = lambda a: a[b:a.shape[0] - b, b:a.shape[1] - b]
    e = np.concatenate([(crop(r) - crop(g))[crop(v)] for r, g, v in zip(rasters, gts, valids)]).astype(np.float32)
    hist, n, key0 = R.histogram(e)
    return R.curve(R.clipped(e), **kw), n


@pytest.mark.parametrize("with_valid", [False, True])
def test_error_distribution_host_path(with_valid):
    scenes, gts, lrs, rs = cpu_scenes()
    b = 2
    valids = [rs.rand(20, 20) < 0.7 if with_valid else np.ones((20, 20), bool) for _ in gts]
    preds = [(g + rs.standard_normal(g.shape) * 2.5).astype(np.float32) for g in gts]
    for p, v in zip(preds, valids):
        p[~v] = -32767.0
    given = [preds[0], preds[1][b:-b, b:-b].copy(), preds[2]]                     # whole and cropped rasters
    got = S.error_distribution(scenes, given, baselines={"COP30": "lr_dem"}, border=0.125, patch_size=16,
                               valid=valids if with_valid else None, gridsize=64, cut=0.25, bw_adjust=0.7)
    assert list(got) == ["SR", "COP30"]
    for name, rasters in (("SR", preds), ("COP30", lrs)):
        (support, dens, (mean, sd, bw)), n = by_hand(rasters, gts, valids, b, gridsize=64, cut=0.25, bw_adjust=0.7)
        g = got[name]
        assert (g["n"], g["n_in"], g["n_below"], g["n_above"]) == n and n[2] + n[3] > 0
        R.check_curve(g["support"], g["density"], support, dens, name)
        assert np.allclose([g["mean"], g["std"], g["bw"]], [mean, sd, bw], rtol=1e-12, atol=0)
    assert got["SR"]["n"] == got["COP30"]["n"] == sum(int(v[b:-b, b:-b].sum()) for v in valids)


def test_degenerate_curves_are_nan():
    key0, K = S.histogram_bins()
    h = torch.zeros((3, K), dtype=torch.int64)
    h[1, 100] = 1                                                                 # n = 1
    h[2, 200] = 50                                                                # no variance
    support, density, stats = S.kde_curves(h, key0)
    assert support.shape == density.shape == (3, 200) and stats.shape == (3, 3)
    assert torch.isnan(support).all() and torch.isnan(density).all()
    v = S.histogram_values(key0, K)
    assert torch.isnan(stats[0]).all() and stats[1, 0] == v[100] and torch.isnan(stats[1, 1:]).all()
    assert stats[2].tolist() == [float(v[200]), 0.0, 0.0]
    s1, d1, st1 = S.kde_curves(h[1], key0, gridsize=7)
    assert s1.shape == d1.shape == (7,) and st1.shape == (3,)


# ---- argument errors -------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    gt = torch.zeros(64)
    win = [(0, 8, 8, (0, 8), [(0, 8)])]
    ok = torch.ones(64, dtype=torch.uint8)
    hist, counts, key0 = S.pooled_histogram([gt], gt, win, valid=ok)
    assert counts.tolist() == [[64, 64, 0, 0]] and hist.sum() == 64
    for bad in (ok.bool(), ok[:63], ok.view(8, 8), np.ones(64, np.uint8)):
        with pytest.raises(ValueError, match="pooled_histogram.*valid"):
            S.pooled_histogram([gt], gt, win, valid=bad)
    with pytest.raises(ValueError, match="candidates"):
        S.pooled_histogram([gt] * 9, gt, [(0, 8, 8, (0, 8), [(0, 8)] * 9)])
    with pytest.raises(ValueError, match="leaves its buffer"):
        S.pooled_histogram([gt], gt, [(0, 8, 8, (8, 8), [(0, 8)])])
    with pytest.raises(ValueError, match="no windows"):
        S.pooled_histogram([gt], gt, [])
    for lo, hi in ((1.0, -1.0), (float("nan"), 1.0), (-1e9, 1.0)):
        with pytest.raises(ValueError, match="lo <= hi"):
            S.pooled_histogram([gt], gt, win, lo, hi)
    for kw in (dict(gridsize=1), dict(cut=-0.1), dict(bw_adjust=0.0), dict(bw_adjust=float("nan"))):
        with pytest.raises(ValueError, match="kde_curves"):
            S.kde_curves(hist, key0, **kw)
    with pytest.raises(ValueError, match="kde_curves"):
        S.kde_curves(hist.float(), key0)
    with pytest.raises(ValueError, match="float16"):
        S.kde_curves(hist, 0xfbff)
    scenes, gts, lrs, rs = cpu_scenes()
    with pytest.raises(ValueError, match="error_distribution.*valid"):
        S.error_distribution(scenes, lrs, border=0.0, patch_size=16, valid=[np.ones((20, 20), bool)] * 2)
    with pytest.raises(ValueError, match="error_distribution: 2 predictions"):
        S.error_distribution(scenes, lrs[:2], border=0.0, patch_size=16)


def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN with a message that names the entry, before a launch or a clear (safe without a GPU: no
    device pointer is dereferenced, the host arrays are real)."""
    lib = _lib.load()
    x, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    labels = (b"errdist_hist", b"errdist_hist (valid)", b"errdist_kde")
    before = {n: lib.jspsr_launch_count(n) for n in labels}
    ptrs, numel = (ctypes.c_void_p * 8)(*[4096] * 8), (ctypes.c_longlong * 8)(*[64] * 8)

    def hist(cands=ptrs, n_cand=1, gt=x, gt_numel=64, valid=x, valid_numel=64, windows=x, n_windows=1, total=64, lo=-5.0, hi=5.0,
             out=x, counts=x):
        return lib.jspsr_errdist_hist_forward(cands, numel, n_cand, gt, gt_numel, valid, valid_numel, windows, n_windows, total, lo, hi,
                                              out, counts, None)

    def message():
        return lib.jspsr_last_error().decode()

    for kw in (dict(cands=None), dict(gt=None), dict(windows=None), dict(out=None), dict(counts=None), dict(n_cand=0), dict(n_cand=9),
               dict(n_windows=0), dict(total=0), dict(gt_numel=0), dict(valid_numel=63), dict(valid_numel=65), dict(total=2 ** 32),
               dict(lo=1.0, hi=0.0), dict(lo=float("nan")), dict(hi=float("inf")), dict(lo=-65505.0)):
        assert hist(**kw) == -1 and "errdist_hist_forward" in message(), kw
    assert hist(valid_numel=63) == -1 and "validity plane" in message()
    nulls = (ctypes.c_void_p * 8)(4096, None, *[4096] * 6)
    assert hist(cands=nulls, n_cand=2) == -1 and "candidate 1" in message()
    for kw in (dict(gt=odd), dict(out=ctypes.c_void_p(4100)), dict(counts=ctypes.c_void_p(4100))):
        assert hist(**kw) == -2 and "aligned" in message() and "errdist_hist_forward" in message(), kw

    def kde(h=x, n_cand=1, key0=S.histogram_bins()[0], K=35330, gridsize=200, cut=0.5, bw_adjust=1.0, support=x, density=x, stats=x, ws=x):
        return lib.jspsr_errdist_kde_forward(h, n_cand, key0, K, gridsize, cut, bw_adjust, support, density, stats, ws, None)

    for kw in (dict(h=None), dict(support=None), dict(density=None), dict(stats=None), dict(ws=None), dict(n_cand=0), dict(n_cand=9),
               dict(K=0), dict(key0=0), dict(K=63489), dict(gridsize=1), dict(cut=-1.0), dict(bw_adjust=0.0), dict(bw_adjust=float("nan"))):
        assert kde(**kw) == -1 and "errdist_kde_forward" in message(), kw
    for kw in (dict(h=ctypes.c_void_p(4100)), dict(ws=ctypes.c_void_p(4104)), dict(density=ctypes.c_void_p(4100))):
        assert kde(**kw) == -2 and "aligned" in message(), kw
    size = lib.jspsr_errdist_workspace_bytes
    assert size(0, 200) == 0 and size(9, 200) == 0 and size(1, 1) == 0 and size(8, 200) >= 8 * 16 and size(1, 2) % 16 == 0
    assert before == {n: lib.jspsr_launch_count(n) for n in labels}


def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert "K21 (ABI v25, additive)" in hdr and "seaborn was not available" in hdr
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\b(?:int|size_t)\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    lib.jspsr_abi_version.restype = ctypes.c_int
    assert lib.jspsr_abi_version() == 25 == _lib.load().jspsr_abi_version()
    assert all(callable(getattr(S, name)) for name in ("pooled_histogram", "histogram_values", "histogram_bins", "kde_curves",
                                                       "error_distribution", "summarise"))
