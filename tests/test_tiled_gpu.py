"""K15 on the MI355X: jspsr_scene_prepare_windows / jspsr_scene_merge_windows and `predict_scenes(tile=...)` through
jspsr_amd.infer, against K13 (`prepare` / `finish`, device against device), the numpy restatements (tests/infer_ref.py,
tests/tiled_ref.py), and `summary.ScenePredictions` / `compose_scene` on the reference's own 3 x 3 cover.

Bounds.  Every window against K13's unpadded frame, every merge against tiled_ref fed with K13's metre values, and every
predict_scenes result against its by-hand composition: == (NaN positions equal).  The DEM against numpy: DEM_TOL of
tests/test_batches_gpu.py.  A pointwise model tiled against untiled: 8 * 2^-24 * max |m| -- a pixel sums at most four
products (m * wx) * wy, two roundings each, with three additions, and the weights sum to 1 within 2^-24."""
import numpy as np
import pytest
import torch

from jspsr_amd import infer as I
from jspsr_amd import summary as S
from jspsr_amd.cover import plan_cover
from tests import batches_ref as B
from tests import tiled_ref as R
from tests.test_infer_gpu import CONFIGS, DEV, KINDS, check_inputs, jspsr_model, launches, params, reference, same, split, store

pytestmark = pytest.mark.gpu

SHAPES = [(70, 91), (64, 120)]
NAN = float("nan")


def window_list(tile):
    """Every tile of a cover of both scenes, interleaved so that neighbours in the batch come from different scenes."""
    kh, kw = (tile, tile) if isinstance(tile, int) else tile
    per = [[(s, y, x) for y, x in plan_cover(h, w, (kh, kw), 8).windows()] for s, (h, w) in enumerate(SHAPES)]
    out = []
    for j in range(max(len(p) for p in per)):
        out += [p[j] for p in per if j < len(p)]
    return out, kh, kw


@pytest.fixture(scope="module")
def two():
    scenes = B.make_scenes(SHAPES, seed=15)
    stores = {}

    def get(i):
        if i not in stores:
            kw, _ = CONFIGS[i]
            Sc = store(scenes, **kw)
            full = [split(I.prepare(Sc, [s], 0, 1)[0], Sc, False) for s in range(2)]            # K13's unpadded frames
            stores[i] = (Sc, full, reference(scenes, params(**kw), 0, 1))
        return stores[i]
    return scenes, get


# ---- prepare_windows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [32, (24, 40), (24, 38)], ids=["32", "24x40", "24x38"])
@pytest.mark.parametrize("config", range(4))
def test_prepare_windows_values(two, config, tile):
    scenes, get = two
    Sc, full, refs = get(config)
    concat = CONFIGS[config][1]
    windows, kh, kw = window_list(tile)
    n0 = launches(b"scene_prepare_windows")
    inputs = I.prepare_windows(Sc, windows, tile, concat=concat)
    assert launches(b"scene_prepare_windows") == n0 + 1
    assert len(inputs) == (1 if concat else 5) and all(t.dtype == torch.float32 and t.is_contiguous() for t in inputs)
    got = split(inputs, Sc, concat)
    assert len({float(b) for b in Sc.base}) == (2 if params(**CONFIGS[config][0])["relative"] else 1)
    for k in KINDS:
        assert got[k].shape == (len(windows), Sc.channels[k], kh, kw)
        for j, (s, y0, x0) in enumerate(windows):                               # device against device, the DEM included
            assert torch.equal(got[k][j], full[s][k][0, :, y0:y0 + kh, x0:x0 + kw]), (config, tile, k, j)
    cut = [{k: v[:, y0:y0 + kh, x0:x0 + kw] for k, v in refs[s].items()} for s, y0, x0 in windows]
    check_inputs(got, cut, (config, tile))                                      # numpy: tests/infer_ref.py's bounds


@pytest.mark.parametrize("guard", [5, 8])
@pytest.mark.parametrize("tile", [32, (24, 38)], ids=["32", "24x38"])
def test_prepare_windows_writes_nothing_outside_its_channels(two, tile, guard):
    """The outputs are channel slices of one larger tensor filled with a sentinel, a spare channel on either side of each
    sample, starting `guard` elements into the allocation (5: no 16-byte alignment, the scalar stores; 8: aligned)."""
    Sc = two[1](0)[0]
    windows, kh, kw = window_list(tile)
    windows = windows[:7]
    want = I.prepare_windows(Sc, windows, tile, concat=True)[0]
    nb, C = want.shape[:2]
    numel = nb * (C + 2) * kh * kw
    big = torch.full((numel + 2 * guard,), -7.0, device=DEV)
    view = big[guard:guard + numel].view(nb, C + 2, kh, kw)
    assert view.data_ptr() == big.data_ptr() + 4 * guard
    outs, c0 = {}, 1
    for k in KINDS:
        outs[k] = (view, c0)
        c0 += Sc.channels[k]
    I.launch_prepare_windows(Sc, I._window_table(Sc, windows), kh, kw, outs)
    assert torch.equal(view[:, 1:C + 1], want)
    assert bool((view[:, 0] == -7.0).all()) and bool((view[:, C + 1] == -7.0).all())
    assert bool((big[:guard] == -7.0).all()) and bool((big[guard + numel:] == -7.0).all())


@pytest.mark.parametrize("tile", [32, (24, 38)], ids=["32", "24x38"])
def test_prepare_windows_over_the_edge_is_nan_exactly_there(two, tile):
    Sc, full, _ = two[1](0)
    kh, kw = (tile, tile) if isinstance(tile, int) else tile
    windows = [(0, 70 - 10, 91 - 13), (1, -5, -3), (0, -kh, 0), (1, 64 - 1, 120 - 1), (1, 8, 120 - kw + 2), (0, 3, 5)]
    got = split(I.prepare_windows(Sc, windows, tile), Sc, False)
    for k in KINDS:
        for j, (s, y0, x0) in enumerate(windows):
            H, W = SHAPES[s]
            want = torch.full((Sc.channels[k], kh, kw), NAN, device=DEV)
            ys, xs = [y for y in range(kh) if 0 <= y0 + y < H], [x for x in range(kw) if 0 <= x0 + x < W]
            if ys and xs:
                want[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = full[s][k][0, :, y0 + ys[0]:y0 + ys[-1] + 1, x0 + xs[0]:x0 + xs[-1] + 1]
            assert same(got[k][j], want), (k, j)
            assert int(torch.isnan(got[k][j]).sum()) == Sc.channels[k] * (kh * kw - len(ys) * len(xs))


def test_prepare_windows_is_cached_and_checks_its_arguments(two):
    Sc = two[1](0)[0]
    windows, _, _ = window_list(32)
    a = I._window_table(Sc, windows)
    assert I._window_table(Sc, list(windows)).data_ptr() == a.data_ptr()        # a repeated call uploads nothing
    with pytest.raises(IndexError):
        I.prepare_windows(Sc, [(2, 0, 0)], 32)
    with pytest.raises(ValueError):
        I.prepare_windows(Sc, [], 32)


# ---- merge_windows -------------------------------------------------------------------------------------------------------
COVERS = [((70, 91), 32, 8, 2), ((64, 120), (24, 40), 10, 0), ((32, 91), 32, 8, 2), ((61, 57), 32, 4, 0)]


def dem_store(shape, elev_log, n=2, seed=31):
    return store(B.make_scenes([shape] * n, seed=seed), kinds=("lr_dem",), coord=None, elev_log=elev_log)


def random_tiles(n, kh, kw, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand((n, 1, kh, kw), generator=g) * 1.4 - 0.2                      # [-0.2, 1.2]: the clamp acts
    t[0, 0, 0, :6] = torch.tensor([0.0, 1.0, -0.0, -0.2, 1.2, 0.5])
    return t.to(DEV).to(dtype)


def metre_tiles(tiles, Sc, idx, cover, metres):
    """`finish`'s values of every tile, each with its scene's base: the frame is the tile."""
    if not metres:
        return tiles.float()[:, 0]
    per = [I.finish(tiles[j * cover.n:(j + 1) * cover.n], Sc, [s] * cover.n, I.Frame(cover.kh, cover.kw, 0, 0, cover.kh, cover.kw))
           for j, s in enumerate(idx)]
    return torch.cat(per)


@pytest.mark.parametrize("metres", [True, False], ids=["metres", "raw"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("elev_log", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("shape,tile,overlap,trim", COVERS, ids=["70x91", "64x120", "one-row", "clip"])
def test_merge_windows_bit_for_bit(shape, tile, overlap, trim, elev_log, dtype, metres):
    Sc = dem_store(shape, elev_log)
    cover = plan_cover(shape[0], shape[1], tile, overlap, trim)
    if shape == (61, 57):
        assert list(cover.oy) == [0, 14, 29] and not cover.wy[2, :3].any()      # the seam clip s_1 = e_0 binds
    if shape == (32, 91):
        assert cover.n_y == 1
    idx = [1, 0]
    assert len({float(np.float32(Sc.base[s])) for s in idx}) == 2
    tiles = random_tiles(2 * cover.n, cover.kh, cover.kw, dtype, seed=shape[0] * shape[1] + overlap)
    n0 = launches(b"scene_merge_windows")
    got = I.merge_windows(tiles, Sc, idx, cover, metres=metres)
    assert launches(b"scene_merge_windows") == n0 + 1
    assert got.dtype == torch.float32 and got.shape == (2,) + shape and bool(torch.isfinite(got).all())
    m = metre_tiles(tiles, Sc, idx, cover, metres).cpu().numpy()
    c = R.cover(shape[0], shape[1], tile, overlap, trim)
    for j in range(2):
        want = R.merge(m[j * cover.n:(j + 1) * cover.n], c)
        assert np.array_equal(got[j].cpu().numpy(), want), (j, np.argwhere(got[j].cpu().numpy() != want)[:4])
    again = I.merge_windows(tiles.view(2, cover.n, cover.kh, cover.kw), Sc, idx, cover, metres=metres)       # the other layout
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))          # two runs, the same bits


@pytest.mark.parametrize("elev_log", [True, False], ids=["log", "linear"])
def test_merge_windows_is_scene_predictions_on_the_reference_cover(elev_log):
    """334 / 128 / 25 / 0: the reference's 3 x 3 cover; K12(a)'s launch and the package's own steps give the same bits."""
    Sc = dem_store((334, 334), elev_log, seed=33)
    cover = plan_cover(334, 334, 128, 25)
    assert list(cover.ox) == [0, 103, 206] and cover.n == 9
    tiles = random_tiles(18, 128, 128, torch.float32, seed=334)
    got = I.merge_windows(tiles, Sc, [0, 1], cover)
    sp = S.ScenePredictions(Sc, 128, 9, border=0.0)
    sp.add(tiles)
    assert sp.complete and torch.equal(got.view(-1), sp.buffer)
    for s in range(2):
        base = torch.tensor(float(np.float32(Sc.base[s])), device=DEV)
        one = S.compose_scene(tiles[9 * s:9 * s + 9], base, 334, 0.0, Sc.elev_min, Sc.elev_max, elev_log)
        assert torch.equal(got[s], one), s


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_merge_windows_does_not_read_a_tile_where_its_weight_is_zero(dtype):
    Sc = dem_store((70, 91), True)
    cover = plan_cover(70, 91, 32, 8, 2)
    tiles = random_tiles(2 * cover.n, 32, 32, dtype, seed=5)
    clean = I.merge_windows(tiles, Sc, [0, 1], cover)
    dead = torch.from_numpy(np.stack([(cover.wy[ty][:, None] == 0) | (cover.wx[tx][None, :] == 0)
                                      for ty in range(cover.n_y) for tx in range(cover.n_x)])).to(DEV)
    assert int(dead.sum()) > 0
    poisoned = tiles.clone()
    poisoned[:, 0][dead.repeat(2, 1, 1)] = NAN
    assert int(torch.isnan(poisoned).sum()) == 2 * int(dead.sum())
    got = I.merge_windows(poisoned, Sc, [0, 1], cover)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)


def test_merge_windows_uploads_its_cover_once_and_checks_its_arguments():
    Sc = dem_store((70, 91), True)
    cover = plan_cover(70, 91, 32, 8, 2)
    a = I._device_cover(cover, Sc.device)
    b = I._device_cover(plan_cover(70, 91, 32, 8, 2), Sc.device)
    assert [t.data_ptr() for t in a] == [t.data_ptr() for t in b]
    assert np.array_equal(a[4].view(torch.float32).cpu().numpy(), cover.wy) and np.array_equal(a[2].cpu().numpy(), cover.lo_y)
    tiles = random_tiles(2 * cover.n, 32, 32, torch.float32, seed=1)
    with pytest.raises(ValueError, match="expected"):
        I.merge_windows(tiles[:-1], Sc, [0, 1], cover)
    with pytest.raises(ValueError, match="fp32 or bf16"):
        I.merge_windows(tiles.half(), Sc, [0, 1], cover)
    with pytest.raises(ValueError, match="a cover of"):
        I.merge_windows(tiles, Sc, [0, 1], plan_cover(64, 91, 32, 8, 2))


# ---- predict_scenes(tile=...) ----------------------------------------------------------------------------------------------
SHAPES4 = [(70, 91), (24, 32), (64, 120), (70, 91)]                             # two shapes, interleaved, and one that fits the tile
TILE, BATCH = 32, 5


@pytest.fixture(scope="module")
def four():
    scenes = B.make_scenes(SHAPES4, seed=44)
    Sc = store(scenes, kinds=("lr_dem", "image", "mask"), coord=None)
    model, _ = jspsr_model()
    return scenes, Sc, model


def by_hand(model, Sc, tiled, tile, batch, overlap, trim, metres=True):
    """prepare_windows -> the model on the same batches -> merge_windows per shape group -> {scene: (H, W)}."""
    covers = {s: plan_cover(*Sc.shapes[s], tile, overlap, trim) for s in tiled}
    windows = [(s, y, x) for s in tiled for y, x in covers[s].windows()]
    preds = []
    with torch.no_grad():
        for lo in range(0, len(windows), batch):
            preds.append(model(*I.prepare_windows(Sc, windows[lo:lo + batch], tile)))
    preds = torch.cat(preds)
    out, at, first = {}, 0, {}
    for s in tiled:
        first[s] = at
        at += covers[s].n
    groups = {}
    for s in tiled:
        groups.setdefault(tuple(Sc.shapes[s]), []).append(s)
    for shape, members in groups.items():
        t = torch.cat([preds[first[s]:first[s] + covers[s].n] for s in members])
        m = I.merge_windows(t, Sc, members, covers[members[0]], metres=metres)
        for j, s in enumerate(members):
            out[s] = m[j]
    return out, preds


def raster(r, pos):
    h, w = r.shapes[pos]
    return r.buffer[r.offsets[pos]:r.offsets[pos] + h * w].view(h, w)


def test_predict_scenes_tiled_equals_the_composition_by_hand(four):
    scenes, Sc, model = four
    n0, m0, f0 = launches(b"scene_prepare_windows"), launches(b"scene_merge_windows"), launches(b"scene_finish")
    r = I.predict_scenes(model, Sc, batch_size=BATCH, tile=TILE, overlap=8, trim=2)
    assert r.shapes == SHAPES4 and r.ids == Sc.ids
    assert launches(b"scene_prepare_windows") == n0 + 8                          # 12 + 15 + 12 windows in batches of 5
    assert launches(b"scene_merge_windows") == m0 + 2 and launches(b"scene_finish") == f0 + 1
    want, _ = by_hand(model, Sc, [0, 2, 3], TILE, BATCH, 8, 2)
    for s in (0, 2, 3):
        assert torch.equal(raster(r, s), want[s]), s
    plain = I.predict_scenes(model, Sc, [1])                                     # the scene that fits: today's path
    assert torch.equal(raster(r, 1), raster(plain, 0))
    assert all(bool(torch.isfinite(raster(r, s)).all()) for s in range(4))
    sub = I.predict_scenes(model, Sc, [3, 2], batch_size=4, tile=TILE, overlap=8, trim=2, metres=False)      # a subset, its order
    want, _ = by_hand(model, Sc, [3, 2], TILE, 4, 8, 2, metres=False)
    assert sub.ids == ["3", "2"] and torch.equal(raster(sub, 0), want[3]) and torch.equal(raster(sub, 1), want[2])
    default = I.predict_scenes(model, Sc, [0], batch_size=BATCH, tile=TILE)      # overlap: a quarter of the tile side
    assert torch.equal(raster(default, 0), by_hand(model, Sc, [0], TILE, BATCH, 8, 0)[0][0])
    m1 = launches(b"scene_merge_windows")
    none = I.predict_scenes(model, Sc, [1, 1], batch_size=2, tile=TILE)          # nothing to tile: no new launch
    assert launches(b"scene_merge_windows") == m1 and torch.equal(raster(none, 1), raster(plain, 0))


class Pointwise(torch.nn.Module):
    """No neighbourhood and no statistics: a tiled run differs from the whole scene by the feathering's roundings alone."""
    name = "jspsr"
    size_multiple = 1

    def forward(self, dem, image, mask):
        return dem * 0.5 + 0.25 * image.mean(1, keepdim=True)


def test_pointwise_model_tiled_is_the_untiled_run_within_the_feathering(four):
    scenes, Sc, _ = four
    model = Pointwise()
    for metres in (True, False):
        whole = I.predict_scenes(model, Sc, [0, 2, 3], batch_size=2, metres=metres)
        for tile, overlap, trim in ((32, 8, 2), ((24, 40), 10, 0), (32, 4, 0)):
            tiled = I.predict_scenes(model, Sc, [0, 2, 3], batch_size=BATCH, tile=tile, overlap=overlap, trim=trim, metres=metres)
            for pos in range(3):
                a, b = raster(tiled, pos).double(), raster(whole, pos).double()
                err, bound = float((a - b).abs().max()), 8 * 2.0 ** -24 * float(b.abs().max())
                print(f"metres {metres} tile {tile} scene {pos}: max |tiled - whole| = {err:.3e}, bound {bound:.3e}")
                assert err <= bound, (metres, tile, pos, err, bound)


class Bf16Out(torch.nn.Module):
    name = "jspsr"
    size_multiple = 8

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, *inputs):
        return self.inner(*inputs).to(torch.bfloat16)


def test_predict_scenes_tiled_bf16(four, monkeypatch):
    scenes, Sc, model = four
    seen = []
    real = I._merge_windows
    monkeypatch.setattr(I, "_merge_windows", lambda tiles, *a, **k: seen.append(tiles.dtype) or real(tiles, *a, **k))
    model.compute_dtype = torch.bfloat16
    try:
        r = I.predict_scenes(model, Sc, [0, 2], batch_size=BATCH, tile=TILE, overlap=8, trim=2)
        want, preds = by_hand(model, Sc, [0, 2], TILE, BATCH, 8, 2)
        assert seen[:2] == [preds.dtype] * 2                                     # the tile buffer has the prediction's dtype
        wrapped = Bf16Out(model)
        del seen[:]
        rb = I.predict_scenes(wrapped, Sc, [0, 2], batch_size=BATCH, tile=TILE, overlap=8, trim=2)
        wantb, predsb = by_hand(wrapped, Sc, [0, 2], TILE, BATCH, 8, 2)
        assert predsb.dtype == torch.bfloat16 and seen[:2] == [torch.bfloat16] * 2
    finally:
        model.compute_dtype = torch.float32
    for pos, s in enumerate((0, 2)):
        assert torch.equal(raster(r, pos), want[s]) and torch.equal(raster(rb, pos), wantb[s]), s
        assert bool(torch.isfinite(raster(r, pos)).all()) and bool(torch.isfinite(raster(rb, pos)).all())


def test_predict_scenes_tiled_argument_errors(four):
    scenes, Sc, model = four
    with pytest.raises(NotImplementedError):
        I.predict_scenes(model, Sc, tile=TILE, tta="d4")
    with pytest.raises(ValueError, match="multiple"):
        I.predict_scenes(model, Sc, tile=36)
    with pytest.raises(ValueError, match="pad must be 0"):
        I.predict_scenes(model, Sc, tile=TILE, pad=4)
    with pytest.raises(ValueError, match="rectangular"):
        I.predict_scenes(model, Sc, tile=(32, 96))                               # (64, 120) clears it, (70, 91) has one side below


def test_predict_scenes_tiled_does_not_synchronise(four, monkeypatch):
    scenes, Sc, model = four
    kw = dict(batch_size=BATCH, tile=TILE, overlap=8, trim=2)
    I.predict_scenes(model, Sc, [0, 1, 2], **kw)                                # warm: tables and covers cached, weights packed
    calls = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self, *a, **k: calls.append("item") or 0)
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append("cpu") or real_cpu(self, *a, **k))
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        r = I.predict_scenes(model, Sc, [0, 1, 2], **kw)
        stop.record()
    assert calls == []
    monkeypatch.undo()
    stream.synchronize()
    rasters = r.rasters()
    assert start.elapsed_time(stop) > 0 and len(rasters) == 3
    want = I.predict_scenes(model, Sc, [0, 1, 2], **kw).rasters()
    assert all(np.array_equal(rasters[k], want[k]) for k in want)
