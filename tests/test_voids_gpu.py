"""K17 on the MI355X: jspsr_scene_nearest_seed, jspsr_scene_fill_voids and jspsr_scene_mask_out through jspsr_amd.infer,
`InferenceScenes(nodata=...)` and `predict_scenes(mask_voids=...)`, against the numpy restatements of tests/voids_ref.py.

Bounds.  Every comparison is bit for bit: the transform is integer arithmetic with a fixed tie rule (np.array_equal on src
and d2), the fill and the mask move fp32 values without arithmetic (int32 views, NaN included), and the composition feeds the
model the same bits in the same batches as the by-hand route (np.array_equal with equal_nan=True for a NaN no-data value)."""
import numpy as np
import pytest
import torch

from jspsr_amd import infer as I
from tests import batches_ref as B
from tests import voids_ref as R
from tests.test_infer_gpu import DEV, jspsr_model, launches, params
from tests.test_tiled_gpu import Pointwise, raster

pytestmark = pytest.mark.gpu

SINGLE = [(1, 1), (1, 7), (7, 1), (5, 9), (33, 63), (33, 64), (33, 65), (33, 130), (150, 20)]     # 150 rows: three bands of 64
THREE = [(5, 9), (33, 130), (64, 64)]
_REFS = {}


def ref(seed, limit=None):
    """tests/voids_ref.py's brute force, computed once per (mask, limit) and left unchanged."""
    key = (seed.shape, seed.tobytes(), limit)
    if key not in _REFS:
        _REFS[key] = R.nearest_seed_ref(seed, limit)
    return _REFS[key]


def masks_for(h, w):
    rs = np.random.RandomState(h * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    out = {}
    for name, (y, x) in (("top left", (0, 0)), ("top right", (0, w - 1)), ("bottom left", (h - 1, 0)), ("bottom right", (h - 1, w - 1))):
        m = np.zeros((h, w), bool)
        m[y, x] = True
        out[name] = m
    out["none"] = np.zeros((h, w), bool)
    out["all"] = np.ones((h, w), bool)
    out["checkerboard"] = (yy + xx) % 2 == 0
    out["random 0.5"] = rs.rand(h, w) < 0.5
    out["random 0.01"] = rs.rand(h, w) < 0.01
    if w > 100:                                                     # a search that crosses a wave and more than one staging pass
        m = rs.rand(h, w) < 0.5
        m[:, 30:100] = False
        out["70 seedless columns"] = m
    if h > 60:                                                      # and one that crosses a band of phase 1
        m = rs.rand(h, w) < 0.5
        m[50:90] = False
        out["40 seedless rows"] = m
    return out


def run(seeds, limit=None):
    """One call over the scenes `seeds` (bool arrays), back to back in one plane -> [(src, d2)] per scene, numpy."""
    shapes = [s.shape for s in seeds]
    plane = torch.from_numpy(np.concatenate([s.reshape(-1) for s in seeds]).astype(np.uint8)).to(DEV)
    n0 = launches(b"scene_nearest_seed")
    src, d2 = I.nearest_seed(plane, shapes, limit)
    assert launches(b"scene_nearest_seed") == n0 + 1
    assert src.dtype == d2.dtype == torch.int32 and src.shape == d2.shape == plane.shape
    src, d2 = src.cpu().numpy(), d2.cpu().numpy()
    out, at = [], 0
    for h, w in shapes:
        out.append((src[at:at + h * w].reshape(h, w), d2[at:at + h * w].reshape(h, w)))
        at += h * w
    return out


@pytest.mark.parametrize("shape", SINGLE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nearest_seed_is_the_rule_exactly(shape):
    for name, seed in masks_for(*shape).items():
        (src, d2), = run([seed])
        want_src, want_d2 = ref(seed)
        assert np.array_equal(d2, want_d2), (shape, name, np.argwhere(d2 != want_d2)[:4].tolist())
        assert np.array_equal(src, want_src), (shape, name, np.argwhere(src != want_src)[:4].tolist())


def test_three_scenes_in_one_launch_never_cross_a_boundary():
    per = [masks_for(h, w) for h, w in THREE]
    for names in (("random 0.5", "random 0.01", "random 0.5"), ("all", "none", "random 0.01"), ("none", "all", "none"),
                  ("bottom right", "70 seedless columns", "40 seedless rows"), ("checkerboard", "top left", "checkerboard")):
        seeds = [p[n] for p, n in zip(per, names)]
        got = run(seeds)
        for j, (src, d2) in enumerate(got):
            want_src, want_d2 = ref(seeds[j])
            assert np.array_equal(src, want_src) and np.array_equal(d2, want_d2), (names, j)
        if "none" in names:                                         # a scene without a seed beside one full of them
            j = names.index("none")
            assert (got[j][0] == -1).all() and (got[j][1] == -1).all()
    # a table with offsets: the scenes in another order than the plane holds them, one left out
    seeds = [per[0]["random 0.5"], per[1]["random 0.5"], per[2]["random 0.5"]]
    plane = torch.from_numpy(np.concatenate([s.reshape(-1) for s in seeds]).astype(np.uint8)).to(DEV)
    table = torch.tensor([[45 + 33 * 130, 64, 64], [0, 5, 9]], dtype=torch.int64, device=DEV)
    src, d2 = I.nearest_seed(plane, table)
    src, d2 = src.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(src[:45].reshape(5, 9), ref(seeds[0])[0]) and np.array_equal(d2[45 + 33 * 130:].reshape(64, 64), ref(seeds[2])[1])


def test_limit():
    for name, seed in masks_for(33, 130).items():
        (src, d2), = run([seed])
        (s3, e3), = run([seed], 3)
        far = (d2 > 9) | (d2 < 0)
        assert (s3[far] == -1).all() and (e3[far] == -1).all(), name
        assert np.array_equal(s3[~far], src[~far]) and np.array_equal(e3[~far], d2[~far]), name
        want = ref(seed, 3)
        assert np.array_equal(s3, want[0]) and np.array_equal(e3, want[1]), name
    tall = masks_for(150, 20)["40 seedless rows"]                   # the limit bounds phase 1's walk over the bands too
    for limit in (1, 19, 20, 64, 65):
        (s, e), = run([tall], limit)
        full = ref(tall)
        far = full[1] > limit * limit
        assert (s[far] == -1).all() and np.array_equal(s[~far], full[0][~far]) and np.array_equal(e[~far], full[1][~far]), limit
    seed = masks_for(33, 130)["random 0.01"]
    (s0, e0), = run([seed], 0)                                      # 0: only the seeds themselves
    assert np.array_equal(e0, np.where(seed, 0, -1)) and np.array_equal(s0, np.where(seed, np.arange(33 * 130).reshape(33, 130), -1))
    (sb, eb), = run([seed], 100000)                                 # beyond every distance: no limit
    assert np.array_equal(sb, ref(seed)[0]) and np.array_equal(eb, ref(seed)[1])
    with pytest.raises(ValueError, match="limit"):
        I.nearest_seed(torch.zeros(9, dtype=torch.uint8, device=DEV), [(3, 3)], limit=1.5)
    with pytest.raises(I._lib.JspsrHipError, match="32767"):
        I.nearest_seed(torch.zeros(40000, dtype=torch.uint8, device=DEV), [(1, 40000)])


def test_sides_of_32767():
    """The largest sides: a row that fills the 64 KB of staging, and a column of 512 bands.  The seeds are regular, so the
    rule's answer is written down directly: the nearest multiple, a tie to the left / to the upper one."""
    n, step = I.MAX_SIDE, 1000
    wide = np.zeros((2, n), bool)
    wide[0, ::step] = True
    (src, d2), = run([wide])
    x = np.arange(n)
    sx = np.minimum((x + step // 2 - 1) // step * step, (n - 1) // step * step)         # x = 500: the seed at 0, not at 1000
    for y in (0, 1):
        assert np.array_equal(src[y], sx) and np.array_equal(d2[y], (sx - x) ** 2 + y * y), y
    tall = np.zeros((n, 3), bool)
    tall[::step, 1] = True
    (src, d2), = run([tall])
    sy = sx
    for c in range(3):
        assert np.array_equal(src[:, c], sy * 3 + 1) and np.array_equal(d2[:, c], (sy - x) ** 2 + (c - 1) ** 2), c
    (s9, e9), = run([tall], 9)                                                  # the limit stops the walk over the bands
    far = d2 > 81
    assert (s9[far] == -1).all() and (e9[far] == -1).all() and np.array_equal(s9[~far], src[~far]) and np.array_equal(e9[~far], d2[~far])


def test_properties_at_200_by_300():
    seed = np.random.RandomState(23).rand(200, 300) < 0.02
    (src, d2), = run([seed])
    assert (src >= 0).all() and seed.reshape(-1)[src].all()         # seed[src] is set
    yy, xx = np.mgrid[0:200, 0:300]
    assert np.array_equal((src // 300 - yy) ** 2 + (src % 300 - xx) ** 2, d2)       # d2 is the distance to src
    assert np.array_equal(d2, R.d2_min_ref(seed))                   # and the minimum over all seeds
    (again_src, again_d2), = run([seed])
    assert np.array_equal(src, again_src) and np.array_equal(d2, again_d2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("limit", [None, 0, 4])
def test_fill_voids_bit_for_bit(limit):
    rs = np.random.RandomState(5)
    shapes = [(5, 9), (33, 130), (64, 64)]
    dems = [rs.uniform(-50, 900, s).astype(np.float32) for s in shapes]
    voids = [rs.rand(*s) < 0.3 for s in shapes]
    voids[1][:, 20:95] = True
    voids[1][4, 60] = False
    for d, v in zip(dems, voids):
        d[v] = np.where(rs.rand(int(v.sum())) < 0.5, np.nan, -32767.0)
    base = np.array([-3.5, 7.25, 100.0], dtype=np.float32)
    dem = torch.from_numpy(np.concatenate([d.reshape(-1) for d in dems])).to(DEV)
    void = torch.from_numpy(np.concatenate([v.reshape(-1) for v in voids]).astype(np.uint8)).to(DEV)
    table = torch.from_numpy(I._host_table(shapes)).to(DEV)
    src = None if limit == 0 else I.nearest_seed(void ^ 1, table, limit)[0]
    n0 = launches(b"scene_fill_voids")
    out = I.fill_voids(dem, void, src, table, torch.from_numpy(base).to(DEV))
    assert launches(b"scene_fill_voids") == n0 + 1 and out.data_ptr() == dem.data_ptr()
    got, at = dem.cpu().numpy(), 0
    assert np.isfinite(got).all()
    for d, v, b in zip(dems, voids, base):
        want = R.fill_ref(d, v, b, limit)
        assert np.array_equal(bits(got[at:at + d.size]), bits(want).reshape(-1)), limit
        at += d.size
    if limit == 4:
        assert (got[45:45 + 33 * 130].reshape(33, 130)[:, 30:85][voids[1][:, 30:85]] == base[1]).sum() > 0     # the base is used


@pytest.mark.parametrize("nodata", [-32767.0, float("nan"), -99999.0])
def test_mask_out_bit_for_bit(nodata):
    rs = np.random.RandomState(9)
    plane = rs.rand(300) < 0.4
    result = rs.uniform(0, 500, 260).astype(np.float32)
    result[7] = np.nan
    rows = np.array([[4, 200, 100], [104, 0, 45], [160, 50, 90]], dtype=np.int64)       # {result offset, plane offset, pixels}
    out = torch.from_numpy(result).to(DEV)
    n0 = launches(b"scene_mask_out")
    I.mask_out(out, torch.from_numpy(plane.astype(np.uint8)).to(DEV), torch.from_numpy(rows).to(DEV), nodata)
    assert launches(b"scene_mask_out") == n0 + 1
    want = result.copy()
    for ro, so, px in rows:
        want[ro:ro + px] = np.where(plane[so:so + px], np.float32(nodata), want[ro:ro + px])
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    bad = torch.tensor([[200, 0, 100], [0, 250, 100], [-1, 0, 5]], dtype=torch.int64, device=DEV)      # rows that leave a buffer
    I.mask_out(out, torch.from_numpy(plane.astype(np.uint8)).to(DEV), bad, nodata)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


# ---- InferenceScenes(nodata=...) -------------------------------------------------------------------------------------------------
SHAPES3 = [(48, 80), (48, 80), (40, 40)]
NODATA = -32767.0
KINDS3 = ("lr_dem", "image", "mask")


def void_scenes(nodata=NODATA):
    """Two 48 x 80 scenes and a 40 x 40 one: a corner void, a disk and speckle, written as the no-data value, NaN and inf."""
    scenes = B.make_scenes(SHAPES3, seed=17)
    rs = np.random.RandomState(71)
    for j, s in enumerate(scenes):
        a = s["lr_dem"] = s["lr_dem"].copy()
        h, w = a.shape[:2]
        yy, xx = np.mgrid[0:h, 0:w]
        v = rs.rand(h, w) < 0.03                                                # speckle everywhere
        if j == 0:
            v[:14, :19] = True                                                  # a corner
        elif j == 1:
            v |= (yy - 22) ** 2 + (xx - 47) ** 2 <= 13 ** 2                     # a disk
        kind = rs.randint(0, 3, (h, w))
        a[..., 0][v] = np.where(kind == 0, nodata, np.where(kind == 1, np.nan, np.inf))[v]
    return scenes


def build(scenes, **kw):
    p = {k: v for k, v in params(**kw).items() if k != "label_range"}
    return I.InferenceScenes(coord=None, device=DEV, **{k: [s[k] for s in scenes] for k in KINDS3}, **p)


@pytest.fixture(scope="module")
def hand():
    """The by-hand route per (relative, void_margin, fill_limit), computed once and left unchanged."""
    scenes, cache = void_scenes(), {}

    def get(relative, margin, limit):
        key = (relative, margin, limit)
        if key not in cache:
            cache[key] = R.by_hand_store([s["lr_dem"] for s in scenes], NODATA, relative, margin, limit)
        return cache[key]
    return scenes, get


@pytest.mark.parametrize("relative", [True, False], ids=["relative", "absolute"])
@pytest.mark.parametrize("margin,limit", [(0, None), (5, None), (0, 0), (5, 4), (0, 4)])
def test_store_is_filled_and_masked_as_by_hand(hand, margin, limit, relative):
    scenes, get = hand
    filled, bases, voids, outs = get(relative, margin, limit)
    n0, f0 = launches(b"scene_nearest_seed"), launches(b"scene_fill_voids")
    S = build(scenes, relative=relative, nodata=NODATA, void_margin=margin, fill_limit=limit)
    assert launches(b"scene_nearest_seed") == n0 + (limit != 0) + (margin > 0) and launches(b"scene_fill_voids") == f0 + 1
    assert [float(np.float32(b)) for b in S.base] == [float(np.float32(b)) for b in bases]
    assert S.void_counts == [int(v.sum()) for v in voids] and min(S.void_counts) > 0
    assert np.array_equal(bits(S.store["lr_dem"].cpu().numpy()), bits(np.concatenate([f.reshape(-1) for f in filled])))
    assert S.void.dtype == torch.uint8 and S.void.shape == (2 * 48 * 80 + 40 * 40,)
    assert (S.void_out is S.void) == (margin == 0)
    for i in range(3):
        assert S.void_mask(i).dtype == torch.bool and np.array_equal(S.void_mask(i).cpu().numpy(), voids[i]), i
        assert np.array_equal(S.void_mask(i, out=True).cpu().numpy(), outs[i]), i
        if margin:
            assert outs[i].sum() > voids[i].sum()
    if limit == 4 and relative:                                                 # the corner is deeper than 4 pixels
        assert float(S.store["lr_dem"][0]) == float(np.float32(bases[0]))


def test_a_store_without_a_void_keeps_its_bits_and_its_predictions():
    scenes = B.make_scenes(SHAPES3, seed=17)
    n0, f0, m0 = launches(b"scene_nearest_seed"), launches(b"scene_fill_voids"), launches(b"scene_mask_out")
    plain, given = build(scenes), build(scenes, nodata=NODATA, void_margin=3, fill_limit=2)
    assert "void" not in plain.__dict__ and plain.void is None
    assert given.void_counts == [0, 0, 0] and not bool(given.void.any()) and given.base == plain.base
    assert all(torch.equal(plain.store[k], given.store[k]) for k in plain.store)
    model = Pointwise()
    for kw in (dict(batch_size=2), dict(batch_size=4, tile=32, overlap=8)):
        a, b = I.predict_scenes(model, plain, **kw), I.predict_scenes(model, given, **kw)
        assert a.offsets == b.offsets and torch.equal(a.buffer.view(torch.int32), b.buffer.view(torch.int32))
    assert (launches(b"scene_nearest_seed"), launches(b"scene_fill_voids"), launches(b"scene_mask_out")) == (n0, f0, m0)


PATHS = {"plain": dict(batch_size=2), "tta": dict(batch_size=8, tta="d4"), "tiled": dict(batch_size=5, tile=32, overlap=8, trim=2),
         "tiled window_tta": dict(batch_size=16, tile=32, overlap=8, trim=2, window_tta="d4")}


@pytest.fixture(scope="module")
def composed(hand):
    """The store with voids and the by-hand store (filled on the host, no nodata, base = the valid minimum), per no-data
    value; the models."""
    scenes, get = hand
    stores = {}

    def pair(nodata, margin):
        key = (repr(nodata), margin)
        if key not in stores:
            src = scenes if nodata == NODATA else void_scenes(nodata)
            filled, bases, voids, outs = get(True, margin, None) if nodata == NODATA else R.by_hand_store(
                [s["lr_dem"] for s in src], nodata, True, margin, None)
            byhand = [dict(s, lr_dem=f) for s, f in zip(src, filled)]
            stores[key] = (build(src, nodata=nodata, void_margin=margin), build(byhand, base=bases), outs)
        return stores[key]
    return pair, {"pointwise": Pointwise(), "jspsr": jspsr_model()[0]}


@pytest.mark.parametrize("path", list(PATHS), ids=list(PATHS))
@pytest.mark.parametrize("model_name", ["pointwise", "jspsr"])
def test_predict_scenes_equals_the_by_hand_route(composed, model_name, path):
    pair, models = composed
    model, kw = models[model_name], PATHS[path]
    for nodata, margin, metres in ((NODATA, 0, True), (NODATA, 5, False)) + (((float("nan"), 5, True),) if path == "plain" else ()):
        S, H, outs = pair(nodata, margin)
        want = I.predict_scenes(model, H, metres=metres, **kw)
        m0 = launches(b"scene_mask_out")
        got = I.predict_scenes(model, S, metres=metres, **kw)
        assert launches(b"scene_mask_out") == m0 + 1                             # one launch for all scenes of the call
        filled = I.predict_scenes(model, S, metres=metres, mask_voids=False, **kw)
        assert launches(b"scene_mask_out") == m0 + 1
        assert got.offsets == want.offsets and got.shapes == want.shapes == SHAPES3
        for pos in range(3):
            w = raster(want, pos).cpu().numpy()
            assert np.isfinite(w).all()
            assert np.array_equal(raster(filled, pos).cpu().numpy(), w), (model_name, path, pos)
            g = raster(got, pos).cpu().numpy()
            assert np.array_equal(g, np.where(outs[pos], np.float32(nodata), w), equal_nan=True), (model_name, path, pos)
            assert (np.isnan(g) if np.isnan(nodata) else g == np.float32(nodata)).sum() == outs[pos].sum()
    sub = I.predict_scenes(model, S, [2, 0], **kw)                               # a subset in its own order
    ref_sub = I.predict_scenes(model, H, [2, 0], **kw)
    for pos, s in enumerate((2, 0)):
        assert np.array_equal(raster(sub, pos).cpu().numpy(), np.where(outs[s], np.float32(nodata), raster(ref_sub, pos).cpu().numpy()),
                              equal_nan=True)


def test_predict_scenes_with_voids_does_not_synchronise(composed, monkeypatch):
    pair, models = composed
    S, _, _ = pair(NODATA, 5)
    kw = dict(batch_size=5, tile=32, overlap=8, trim=2)
    model = models["pointwise"]
    want = I.predict_scenes(model, S, **kw).rasters()                            # warm: tables and covers cached
    uploads = len(S._infer_tables)
    calls = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self, *a, **k: calls.append("item") or 0)
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append("cpu") or real_cpu(self, *a, **k))
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        r = I.predict_scenes(model, S, **kw)
    assert calls == [] and len(S._infer_tables) == uploads
    monkeypatch.undo()
    stream.synchronize()
    got = r.rasters()
    assert all(np.array_equal(got[k], want[k]) for k in want)
