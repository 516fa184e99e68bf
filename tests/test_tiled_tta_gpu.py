"""K16 on the MI355X: jspsr_scene_prepare_windows_d4, `mean_windows` and `predict_scenes(tile=..., window_tta=...)` through
jspsr_amd.infer, against what K15 and K14 already pin: `prepare_windows`' output moved by torch.rot90 / torch.flip on the
device, the numpy mean of tests/tiled_tta_ref.py, and the composition by hand from the public pieces.

Bounds.  Every comparison is bit for bit (int32 views, NaN included, or torch.equal) but one: the index maps are integers,
the per-kind arithmetic is the shared csrc/totensor.h, the mean is a fixed sequence of fp32 operations, and the model sees
the same bits in the same batches.  The exception is a pointwise model under "d4" against the plain tiled pass,
metres=False: all K predictions carried back are bit-equal, v say; of the K - 1 sequential fp32 additions the first, v + v,
is exact, the others and the one division round once each, 2^-24 relative: K - 1 roundings, within K * 2^-24; the
feathering adds the 8 * 2^-24 of tests/test_tiled_gpu.py: max |a - b| <= (K + 8) * 2^-24 * max |b|."""
import numpy as np
import pytest
import torch

from jspsr_amd import infer as I
from jspsr_amd.cover import plan_cover
from tests import batches_ref as B
from tests import tiled_tta_ref as R
from tests.test_infer_gpu import CONFIGS, DEV, KINDS, jspsr_model, launches, split, store
from tests.test_tiled_gpu import SHAPES, SHAPES4, Bf16Out, Pointwise, raster, window_list
from tests.test_tta_gpu import ELEMENT_SETS, Stub, same_bits

pytestmark = pytest.mark.gpu

TILES = [32, (24, 40), (24, 38), (38, 24), (40, 72)]
TILE_IDS = ["32", "24x40", "24x38", "38x24", "40x72"]
D4 = I.d4_elements("d4")
THREE = [(1, False, False), (0, True, False), 10]                               # 10 = (2, True, False)
NAN = float("nan")


def same_rasters(a, b):
    """Every scene's raster bit for bit (the buffer's alignment gaps between shape groups are not written)."""
    return a.offsets == b.offsets and a.shapes == b.shapes and all(
        torch.equal(raster(a, pos).view(torch.int32), raster(b, pos).view(torch.int32)) for pos in range(len(a.shapes)))


def turned(t, element):
    """flipud?(fliplr?(rot90(t, rot90))) over the last two dimensions, on the device."""
    r, lr, ud = I._element(element)
    t = torch.rot90(t, r, dims=(-2, -1))
    t = torch.flip(t, dims=(-1,)) if lr else t
    return (torch.flip(t, dims=(-2,)) if ud else t).contiguous()


@pytest.fixture(scope="module")
def two():
    scenes = B.make_scenes(SHAPES, seed=15)
    stores, upright = {}, {}

    def get(i):
        if i not in stores:
            stores[i] = store(scenes, **CONFIGS[i][0])
        return stores[i]

    def up(i, windows, tile):
        """`prepare_windows`' output per kind, computed once per (store, tile) and left unchanged."""
        key = (i, tile, tuple(windows))
        if key not in upright:
            upright[key] = split(I.prepare_windows(get(i), windows, tile), get(i), False)
        return upright[key]
    return get, up


# ---- prepare_windows_d4 ----------------------------------------------------------------------------------------------------
def test_torch_and_numpy_turn_the_same_way():
    a = np.arange(35, dtype=np.float32).reshape(1, 5, 7)
    for code in range(16):
        assert np.array_equal(turned(torch.from_numpy(a).to(DEV), code).cpu().numpy(), R.window_transform(a, code)), code


@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
@pytest.mark.parametrize("config", range(4))
def test_prepare_windows_d4_values(two, config, tile):
    get, up = two
    Sc, concat = get(config), CONFIGS[config][1]
    windows, kh, kw = window_list(tile)
    N = len(windows)
    assert {s for s, _, _ in windows[:2]} == {0, 1}                              # neighbours in the batch from different scenes
    want = up(config, windows, tile)
    n0 = launches(b"scene_prepare_windows_d4")
    groups = I.prepare_windows_d4(Sc, windows, tile, "d4", concat=concat)
    assert launches(b"scene_prepare_windows_d4") == n0 + 2 and sorted(groups) == [0, 1]     # one launch per parity
    for parity, (inputs, order) in groups.items():
        es = [e for e in D4 if e[0] % 2 == parity]
        oh, ow = (kw, kh) if parity else (kh, kw)
        assert order == [(j, e) for e in es for j in range(N)]
        assert len(inputs) == (1 if concat else 5) and all(t.dtype == torch.float32 and t.is_contiguous() for t in inputs)
        got = split(inputs, Sc, concat)
        for k in KINDS:
            assert got[k].shape == (4 * N, Sc.channels[k], oh, ow), (k, got[k].shape)
            for m, e in enumerate(es):
                g, w = got[k][m * N:(m + 1) * N], turned(want[k], e)
                assert same_bits(g, w), (config, tile, k, e, (g.contiguous().view(torch.int32) != w.view(torch.int32)).nonzero()[:4].tolist())


@pytest.mark.parametrize("tile", [32, (24, 38)], ids=["32", "24x38"])
def test_one_launch_mixes_even_codes_and_scenes(two, tile):
    get, up = two
    Sc = get(0)
    windows, kh, kw = window_list(tile)
    windows = windows[:8]
    codes = [0, 2, 8, 10, 10, 8, 2, 0]
    base = I._window_rows(Sc, windows)
    table = torch.from_numpy(np.concatenate([base, np.array(codes, np.int32)[:, None]], axis=1)).to(DEV)
    outs = {k: (torch.full((8, Sc.channels[k], kh, kw), -7.0, device=DEV), 0) for k in KINDS}
    n0 = launches(b"scene_prepare_windows_d4")
    I.launch_prepare_windows_d4(Sc, table, codes, kh, kw, outs)
    assert launches(b"scene_prepare_windows_d4") == n0 + 1
    for code in (0, 2, 8, 10):
        alone = split(I.prepare_windows_d4(Sc, windows, tile, [code])[0][0], Sc, False)     # a launch of its own
        for k in KINDS:
            for j in [j for j in range(8) if codes[j] == code]:
                assert same_bits(outs[k][0][j], alone[k][j]), (code, k, j)
                assert same_bits(outs[k][0][j], turned(up(0, tuple(windows), tile)[k][j], code)), (code, k, j)
    # a device table whose code is outside 0..15 or of the other parity, or that names no scene, gives NaN samples
    bad = table[:4].clone()
    bad[1, 4], bad[2, 4], bad[3, 0] = 4, 16, 5
    out = torch.full((4, 1, kh, kw), -7.0, device=DEV)
    I.launch_prepare_windows_d4(Sc, bad, [0, 2, 8, 10], kh, kw, {"lr_dem": (out, 0)})
    assert same_bits(out[0], outs["lr_dem"][0][0]) and bool(torch.isnan(out[1:]).all())


@pytest.mark.parametrize("element", [(0, True, False), (2, False, False), (1, True, False), (3, False, True)], ids=str)
@pytest.mark.parametrize("tile", [32, (24, 38)], ids=["32", "24x38"])
def test_over_the_edge_is_nan_exactly_at_the_transformed_places(two, tile, element):
    get, up = two
    Sc = get(0)
    kh, kw = (tile, tile) if isinstance(tile, int) else tile
    windows = ((0, 70 - 10, 91 - 13), (1, -5, -3), (0, -kh, 0), (1, 64 - 1, 120 - 1), (1, 8, 120 - kw + 2), (0, 3, 5))
    want = up(0, windows, tile)
    (inputs, order), = I.prepare_windows_d4(Sc, windows, tile, [element]).values()
    got = split(inputs, Sc, False)
    for k in KINDS:
        w = turned(want[k], element)
        assert same_bits(got[k], w), (k, element)                               # prepare_windows' bits everywhere else
        assert torch.equal(torch.isnan(got[k]), turned(torch.isnan(want[k]), element))
        for j, (s, y0, x0) in enumerate(windows):                               # and the count, from the geometry alone
            H, W = SHAPES[s]
            inside = len([y for y in range(kh) if 0 <= y0 + y < H]) * len([x for x in range(kw) if 0 <= x0 + x < W])
            assert int(torch.isnan(got[k][j]).sum()) == Sc.channels[k] * (kh * kw - inside), (k, j)
    assert bool(torch.isnan(got["lr_dem"][2]).all()) and not bool(torch.isnan(got["lr_dem"][5]).any())


@pytest.mark.parametrize("guard", [5, 8])
@pytest.mark.parametrize("parity", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("tile", [32, (24, 38)], ids=["32", "24x38"])
def test_prepare_windows_d4_writes_nothing_outside_its_channels(two, tile, parity, guard):
    """The outputs are channel slices of one larger tensor filled with a sentinel, a spare channel on either side of each
    sample, starting `guard` elements into the allocation (5: no 16-byte alignment, the scalar stores; 8: aligned)."""
    get, _ = two
    Sc = get(0)
    windows, kh, kw = window_list(tile)
    windows = windows[:3]
    elements = [(parity, False, False), (parity + 2, True, False)]
    want = I.prepare_windows_d4(Sc, windows, tile, elements, concat=True)[parity][0][0]
    nb, C, oh, ow = want.shape
    assert (nb, oh, ow) == (6,) + ((kw, kh) if parity else (kh, kw))
    numel = nb * (C + 2) * oh * ow
    big = torch.full((numel + 2 * guard,), -7.0, device=DEV)
    view = big[guard:guard + numel].view(nb, C + 2, oh, ow)
    assert view.data_ptr() == big.data_ptr() + 4 * guard
    outs, c0 = {}, 1
    for k in KINDS:
        outs[k] = (view, c0)
        c0 += Sc.channels[k]
    table, host = I._window_table_d4(Sc, windows, [I.d4_code(e) for e in elements])
    assert I._window_table_d4(Sc, list(windows), [I.d4_code(e) for e in elements])[0].data_ptr() == table.data_ptr()   # cached
    I.launch_prepare_windows_d4(Sc, table, host, kh, kw, outs)
    assert same_bits(view[:, 1:C + 1], want)
    assert bool((view[:, 0] == -7.0).all()) and bool((view[:, C + 1] == -7.0).all())
    assert bool((big[:guard] == -7.0).all()) and bool((big[guard + numel:] == -7.0).all())


# ---- mean_windows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tile", [32, (24, 40)], ids=["32", "24x40"])
def test_mean_windows_bit_for_bit(tile, dtype):
    kh, kw = (tile, tile) if isinstance(tile, int) else tile
    g = torch.Generator().manual_seed(kh * 100 + kw)
    N = 5
    for K, elements in ELEMENT_SETS.items():
        preds = []
        for e in elements:
            oh, ow = (kw, kh) if e[0] % 2 else (kh, kw)
            preds.append((torch.rand((N, 1, oh, ow), generator=g) * 1.4 - 0.2).to(DEV).to(dtype))      # [-0.2, 1.2]
        n0 = launches(b"scene_finish_mean")
        got = I.mean_windows(preds, elements, tile)
        assert launches(b"scene_finish_mean") == n0 + 1
        assert got.dtype == torch.float32 and got.shape == (N, 1, kh, kw)
        want = R.mean_tiles([R.carried_back(p.float().cpu().numpy()[:, 0], e) for p, e in zip(preds, elements)])
        assert same_bits(got[:, 0], want), (K, tile, dtype)
        if K == 1:                                                              # the identity alone: the input, widened
            assert same_bits(got, preds[0].float())
    with pytest.raises(ValueError, match="expected"):
        I.mean_windows([preds[0][:, :, :-1]], [0], tile)
    with pytest.raises(ValueError, match="predictions for"):
        I.mean_windows(preds[:2], [0], tile)


# ---- predict_scenes(tile=..., window_tta=...) -----------------------------------------------------------------------------------
def by_hand(model, Sc, tiled, tile, elements, batch, overlap, trim, metres=True):
    """The public pieces: prepare_windows -> torch transforms -> the model, in predict_scenes' batches (chunks of nb windows,
    each set of elements in forwards of `per`, even before odd, element-major) -> mean_windows -> merge_windows per shape
    group -> {scene: (H, W)}."""
    elements = I.d4_elements(elements)
    kh, kw = I._tile_sides(tile)
    covers = {s: plan_cover(*Sc.shapes[s], tile, overlap, trim) for s in tiled}
    windows = [(s, y, x) for s in tiled for y, x in covers[s].windows()]
    even, odd = [e for e in elements if e[0] % 2 == 0], [e for e in elements if e[0] % 2 == 1]
    sets = [even + odd] if kh == kw else [s for s in (even, odd) if s]
    nb = max(1, batch // max(len(s) for s in sets))
    per = max(1, batch // nb)
    means, chunks = [], 0
    with torch.no_grad():
        for lo in range(0, len(windows), nb):
            up = I.prepare_windows(Sc, windows[lo:lo + nb], tile)
            n = up[0].shape[0]
            preds = {}
            for s in sets:
                for e0 in range(0, len(s), per):
                    run = s[e0:e0 + per]
                    pred = model(*[torch.cat([turned(t, e) for e in run]) for t in up])
                    assert pred.shape[0] == n * len(run) <= max(batch, n)
                    for j, e in enumerate(run):
                        preds[e] = pred[j * n:(j + 1) * n]
            means.append(I.mean_windows([preds[e] for e in elements], elements, tile))
            chunks += 1
    means = torch.cat(means)
    assert means.dtype == torch.float32
    out, at, first = {}, 0, {}
    for s in tiled:
        first[s] = at
        at += covers[s].n
    groups = {}
    for s in tiled:
        groups.setdefault(tuple(Sc.shapes[s]), []).append(s)
    for shape, members in groups.items():
        t = torch.cat([means[first[s]:first[s] + covers[s].n] for s in members])
        m = I.merge_windows(t, Sc, members, covers[members[0]], metres=metres)
        for j, s in enumerate(members):
            out[s] = m[j]
    return out, chunks, len(groups)


@pytest.fixture(scope="module")
def stubbed():
    scenes = B.make_scenes(SHAPES4, seed=44)
    return store(scenes, kinds=("lr_dem", "image"), coord=None), Stub().to(DEV)


@pytest.mark.parametrize("elements", ["d4", THREE], ids=["d4", "three"])
@pytest.mark.parametrize("tile", [32, (24, 40)], ids=["32", "24x40"])
@pytest.mark.parametrize("batch_size", [5, 16])
def test_predict_scenes_window_tta_equals_the_composition_by_hand(stubbed, batch_size, tile, elements):
    Sc, model = stubbed
    kw = dict(batch_size=batch_size, model_name="jspsr")
    want, chunks, n_groups = by_hand(model, Sc, [0, 2, 3], tile, elements, batch_size, 8, 2)
    whole = I.predict_scenes(model, Sc, [1], tta=elements, **kw)                # the scene that fits: K14's path, one launch
    n0, m0, p0 = launches(b"scene_finish_mean"), launches(b"scene_merge_windows"), launches(b"scene_prepare_windows")
    r = I.predict_scenes(model, Sc, tile=tile, overlap=8, trim=2, window_tta=elements, **kw)
    assert r.shapes == SHAPES4 and r.ids == Sc.ids
    assert launches(b"scene_finish_mean") == n0 + chunks + 1                    # one per chunk, and the untiled scene's
    assert launches(b"scene_merge_windows") == m0 + n_groups == m0 + 2 and launches(b"scene_prepare_windows") == p0
    for s in (0, 2, 3):
        assert torch.equal(raster(r, s), want[s]), (batch_size, tile, s)
    assert torch.equal(raster(r, 1), raster(whole, 0))
    assert all(bool(torch.isfinite(raster(r, s)).all()) for s in range(4))
    plain = I.predict_scenes(model, Sc, tile=tile, overlap=8, trim=2, **kw)
    assert not torch.equal(raster(plain, 0), raster(r, 0))                      # the stub is not equivariant: the ensemble shows
    if tile == 32 and elements == "d4":                                         # a subset in its own order, the network's range
        sub = I.predict_scenes(model, Sc, [3, 2], tile=tile, overlap=8, trim=2, window_tta=elements, metres=False, **kw)
        want, _, _ = by_hand(model, Sc, [3, 2], tile, elements, batch_size, 8, 2, metres=False)
        assert sub.ids == ["3", "2"] and torch.equal(raster(sub, 0), want[3]) and torch.equal(raster(sub, 1), want[2])


@pytest.fixture(scope="module")
def four():
    scenes = B.make_scenes(SHAPES4, seed=44)
    Sc = store(scenes, kinds=("lr_dem", "image", "mask"), coord=None)
    model, _ = jspsr_model()
    return Sc, model


@pytest.mark.parametrize("compute", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_predict_scenes_window_tta_with_jspsr(four, compute):
    Sc, model = four
    elements = [(0, False, False), (1, True, False)]
    kw = dict(batch_size=8, tile=32, overlap=8, trim=2)
    model.compute_dtype = compute
    try:
        r = I.predict_scenes(model, Sc, [0, 1, 2], window_tta=elements, **kw)
        again = I.predict_scenes(model, Sc, [0, 1, 2], window_tta=elements, **kw)
        want, chunks, _ = by_hand(model, Sc, [0, 2], 32, elements, 8, 8, 2)
        plain = I.predict_scenes(model, Sc, [0, 1, 2], **kw)
        fits = I.predict_scenes(model, Sc, [1], batch_size=8, tta=elements)
    finally:
        model.compute_dtype = torch.float32
    assert chunks == 7                                                          # 12 + 15 windows, four to a chunk
    assert same_rasters(r, again)                                               # two runs, the same bits
    assert all(bool(torch.isfinite(raster(r, pos)).all()) for pos in range(3))
    for pos, s in ((0, 0), (2, 2)):
        assert torch.equal(raster(r, pos), want[s]), (compute, s)
        assert not torch.equal(raster(r, pos), raster(plain, pos))
    assert torch.equal(raster(r, 1), raster(fits, 0))


def test_the_identity_alone_is_the_plain_tiled_pass(stubbed, four):
    Sc, model = stubbed
    for bs in (5, 16):
        kw = dict(batch_size=bs, tile=32, overlap=8, trim=2, model_name="jspsr")
        a, b = I.predict_scenes(model, Sc, window_tta=[(0, False, False)], **kw), I.predict_scenes(model, Sc, **kw)
        assert same_rasters(a, b), bs
    Sc, model = four
    for m in (model, Bf16Out(model)):                                           # an fp32 copy of bf16 predictions is exact
        kw = dict(batch_size=5, tile=32, overlap=8, trim=2)
        a, b = I.predict_scenes(m, Sc, [0, 1, 2], window_tta=[0], **kw), I.predict_scenes(m, Sc, [0, 1, 2], **kw)
        assert same_rasters(a, b), type(m).__name__


def test_pointwise_model_under_d4_is_the_plain_tiled_pass_within_the_mean(four):
    Sc, _ = four
    model = Pointwise()
    K = len(D4)
    for tile, overlap, trim in ((32, 8, 2), ((24, 40), 10, 0)):
        kw = dict(batch_size=16, tile=tile, overlap=overlap, trim=trim, metres=False)
        plain = I.predict_scenes(model, Sc, [0, 2, 3], **kw)
        tta = I.predict_scenes(model, Sc, [0, 2, 3], window_tta="d4", **kw)
        for pos in range(3):
            a, b = raster(tta, pos).double(), raster(plain, pos).double()
            err, bound = float((a - b).abs().max()), (K + 8) * 2.0 ** -24 * float(b.abs().max())
            print(f"tile {tile} scene {pos}: max |window_tta - plain| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (tile, pos, err, bound)


def test_predict_scenes_window_tta_does_not_synchronise(four, monkeypatch):
    Sc, model = four
    kw = dict(batch_size=8, tile=32, overlap=8, trim=2, window_tta=[(0, False, False), (1, True, False), (2, False, False)])
    I.predict_scenes(model, Sc, [0, 1, 2], **kw)                                # warm: tables and covers cached, weights packed
    uploads = len(Sc._infer_tables)
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
    assert calls == [] and len(Sc._infer_tables) == uploads                     # nothing uploaded again either
    monkeypatch.undo()
    stream.synchronize()
    rasters = r.rasters()
    assert start.elapsed_time(stop) > 0 and len(rasters) == 3
    want = I.predict_scenes(model, Sc, [0, 1, 2], **kw).rasters()
    assert all(np.array_equal(rasters[k], want[k]) for k in want)
