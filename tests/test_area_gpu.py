"""K26 on the MI355X: jspsr_area_forward through `resample.area_rasters` / `area_resize` and the stores built with
`guide_resample="area"`, against the numpy int64 restatement tests/area_ref.py.  Every comparison is integer equality.

The shapes are the smallest at which the kernel can still go wrong: a wave owns 16 output rows by 64 output columns and reads
the source row under them in chunks of 4080 // C pixels, so the outputs cross 16 rows and 64 columns with full, ragged and
single-column units, and the rows of some cases are longer than one chunk."""
import ctypes

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import infer as I
from jspsr_amd import resample as RS
from tests import area_ref as A
from tests import batches_ref as B
from tests.test_infer_gpu import DEV, jspsr_model, launches, params

pytestmark = pytest.mark.gpu

# (h, w) -> (H, W), C: the axes 8->8, 16->8, 15->5, 15->4, 65->64, 129->2, 64->4, 173->10 and 300->1 paired so that both vary
RATIOS = [((8, 16), (8, 8), 3), ((15, 15), (5, 4), 1), ((65, 129), (64, 2), 4), ((64, 173), (4, 10), 3), ((300, 65), (1, 64), 15),
          ((173, 300), (10, 1), 16), ((16, 64), (8, 4), 4), ((129, 15), (2, 5), 3),
          ((9, 63), (9, 9), 3), ((63, 9), (9, 9), 3)]                          # ratio 1 on one axis and 7 on the other
# output heights and widths 1, 63, 64, 65, 129 at ratios of 1.5 and 2 and a bit
EDGES = [((2, 259), (1, 129), 3), ((95, 131), (63, 65), 3), ((96, 129), (64, 64), 3), ((98, 127), (65, 63), 3), ((194, 3), (129, 1), 3),
         ((97, 130), (64, 65), 1), ((40, 259), (17, 129), 4)]
# rows longer than one chunk of the wave's buffer (1360 pixels of 3 channels, 255 of 16), and 65 columns of them
LONG = [((7, 3001), (2, 64), 3), ((20, 1300), (3, 65), 16), ((5, 4500), (5, 2), 1)]
CHANNELS = [((37, 53), (10, 14), c) for c in (1, 3, 4, 15, 16)]
CASES = RATIOS + EDGES + LONG + CHANNELS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV)


def one(a, dst, mode="area"):
    h, w, C = a.shape
    out, table = RS.area_rasters(dev(a), [(0, h, w)], C, [dst], mode)
    assert table.tolist() == [[0, *dst]] and out.dtype == torch.uint8 and out.numel() == dst[0] * dst[1] * C
    return out.cpu().numpy().reshape(*dst, C)


@pytest.mark.parametrize("src,dst,C", CASES, ids=[f"{s[0]}x{s[1]}x{c}-{d[0]}x{d[1]}" for s, d, c in CASES])
def test_area_is_the_restatement(src, dst, C):
    a = np.random.default_rng(src[0] * 1000 + src[1] + C).integers(0, 256, (*src, C), dtype=np.uint8)
    n0 = launches(b"area")
    got = one(a, dst)
    assert launches(b"area") == n0 + 1
    assert np.array_equal(got, A.area_u8(a, *dst))
    if src == dst:
        assert np.array_equal(got, a)


def test_values():
    for v in (0, 255):
        for src, dst, C in (((15, 15), (4, 4), 3), ((65, 130), (64, 65), 1)):
            assert np.all(one(np.full((*src, C), v, np.uint8), dst) == v), (v, src)
    yy, xx = np.mgrid[0:66, 0:131]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None].repeat(3, axis=2)
    board[..., 1] = 255 - board[..., 1]
    for dst in ((33, 65), (17, 35), (66, 131), (1, 1)):
        assert np.array_equal(one(board, dst), A.area_u8(board, *dst)), dst
    halves = {(0, 0, 0, 2): 1, (1, 0, 0, 0): 0, (1, 1, 0, 0): 1, (255, 255, 255, 254): 255}      # round half up, on 2 x 2 blocks
    blocks = np.zeros((2 * len(halves), 2 * 70, 1), np.uint8)
    for j, b in enumerate(halves):
        blocks[2 * j:2 * j + 2] = np.tile(np.uint8(b).reshape(2, 2, 1), (1, 70, 1))
    got = one(blocks, (len(halves), 70))
    for j, want in enumerate(halves.values()):
        assert np.all(got[j] == want), (j, want)
    assert np.array_equal(got, A.area_u8(blocks, len(halves), 70))


@pytest.fixture(scope="module")
def five():
    """Five rasters of three channels at odd pixel offsets (no raster starts on a dword), their shapes and restatements."""
    rng = np.random.default_rng(26)
    shapes = [((15, 17), (4, 5)), ((65, 67), (64, 3)), ((9, 131), (9, 65)), ((33, 35), (33, 35)), ((173, 21), (10, 1))]
    rasters = [rng.integers(0, 256, (*s, 3), dtype=np.uint8) for s, _ in shapes]
    offs, o = [], 1                                                              # one pixel of padding in front: 3 bytes
    for (h, w), _ in shapes:
        assert o % 2 == 1 and h * w % 2 == 1
        offs.append(o)
        o += h * w + 1                                                           # and one between the rasters
    flat = rng.integers(0, 256, o * 3, dtype=np.uint8)
    for a, off in zip(rasters, offs):
        flat[off * 3:(off + a.shape[0] * a.shape[1]) * 3] = a.reshape(-1)
    want = [A.area_u8(a, *d) for a, (_, d) in zip(rasters, shapes)]
    return shapes, rasters, offs, flat, want


def test_five_rasters_off_the_dword_grid_in_one_call_and_the_guards(five):
    shapes, rasters, offs, flat, want = five
    table = [(o, *s) for o, (s, _) in zip(offs, shapes)]
    n0 = launches(b"area")
    out, dt = RS.area_rasters(dev(flat), table, 3, [d for _, d in shapes])
    assert launches(b"area") == n0 + 1
    sizes = [d[0] * d[1] for _, d in shapes]
    assert dt[:, 0].tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist() and out.numel() == 3 * sum(sizes)   # no gap
    got = out.cpu().numpy()
    for k, (o, H, W) in enumerate(dt.tolist()):
        assert np.array_equal(got[3 * o:3 * (o + H * W)].reshape(H, W, 3), want[k]), k
    # the raw entry into a buffer with guards: the results from pixel 5 on, nothing before or after them written
    lib = _lib.load()
    front, back = 5, 7
    rows = np.zeros((5, 6), dtype=np.int64)
    rows[:, 0:3] = table
    rows[:, 4:6] = [d for _, d in shapes]
    rows[:, 3] = front + dt[:, 0]
    total = front + sum(sizes) + back
    dst = torch.full((total * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    src, dtab = dev(flat), torch.from_numpy(rows).to(DEV)
    assert lib.jspsr_area_forward(src.data_ptr(), flat.size // 3, dst.data_ptr(), total, dtab.data_ptr(), rows.ctypes.data, 5, 3, 0,
                                  torch.cuda.current_stream().cuda_stream) == 0
    raw = dst.cpu().numpy()
    assert np.all(raw[:front * 3] == 0xA5) and np.all(raw[(front + sum(sizes)) * 3:] == 0xA5)
    assert np.array_equal(raw[front * 3:(front + sum(sizes)) * 3], got)


def test_determinism_alone_and_in_company(five):
    shapes, rasters, offs, flat, want = five
    table = [(o, *s) for o, (s, _) in zip(offs, shapes)]
    runs = [RS.area_rasters(dev(flat), table, 3, [d for _, d in shapes])[0] for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    for k, (a, (_, d)) in enumerate(zip(rasters, shapes)):
        assert np.array_equal(one(a, d), want[k]), k


@pytest.mark.parametrize("rows", [1040, 520, 260])
def test_every_band_height(rows):
    """The entry halves the 16 output rows of a unit while the call has fewer than 2048 units, so a small call runs with bands
    of 2.  A blank raster of rows x 2112 in the same call (65 x 33, then 2 x 33 x 33 units ...) keeps the band at 16, 8 and 4;
    the bytes of the raster beside it do not change."""
    a = np.random.default_rng(rows).integers(0, 256, (173, 300, 3), dtype=np.uint8)
    flat = torch.zeros(a.size + rows * 2112 * 3, dtype=torch.uint8, device=DEV)
    flat[:a.size] = dev(a)
    out, table = RS.area_rasters(flat, [(0, 173, 300), (173 * 300, rows, 2112)], 3, [(50, 70), (rows, 2112)])
    assert table.tolist() == [[0, 50, 70], [3500, rows, 2112]]
    assert np.array_equal(out[:10500].cpu().numpy().reshape(50, 70, 3), A.area_u8(a, 50, 70)) and not bool(out[10500:].any())


def test_unaligned_buffers_of_four_and_sixteen_channels():
    """C % 4 == 0 reads and writes whole words where src and dst allow it, and bytes from a view that starts off a word."""
    rng = np.random.default_rng(4)
    for C in (4, 16):
        a = rng.integers(0, 256, (37, 150, C), dtype=np.uint8)
        want = A.area_u8(a, 10, 66)
        assert np.array_equal(one(a, (10, 66)), want)
        for lead in (1, 2, 3, 5):
            buf = torch.zeros(a.size + lead, dtype=torch.uint8, device=DEV)
            buf[lead:] = dev(a)
            view = buf[lead:]
            assert view.data_ptr() % 4 == lead % 4
            out, _ = RS.area_rasters(view, [(0, 37, 150)], C, [(10, 66)])
            assert np.array_equal(out.cpu().numpy().reshape(10, 66, C), want), (C, lead)


def test_area_resize_takes_a_batch():
    a = np.random.default_rng(8).integers(0, 256, (3, 30, 41, 3), dtype=np.uint8)
    x = torch.from_numpy(a).to(DEV)
    got = RS.area_resize(x, (8, 11))
    assert got.shape == (3, 8, 11, 3) and got.dtype == torch.uint8
    for b in range(3):
        assert np.array_equal(got[b].cpu().numpy(), A.area_u8(a[b], 8, 11)), b
    with pytest.raises(ValueError, match="upsampling"):
        RS.area_resize(x, (31, 41))
    with pytest.raises(ValueError, match="upsampling"):
        RS.area_rasters(x.view(-1), [(0, 90, 41)], 3, [(8, 42)])
    with pytest.raises(ValueError, match="not inside"):
        RS.area_rasters(x.view(-1), [(1, 90, 41)], 3, [(8, 11)])
    with pytest.raises(ValueError, match="mode"):
        RS.area_resize(x, (8, 11), mode="nearest")


def test_wide_accumulator():
    """S passes 2^32: 4112 x 4112 pixels of 255 under one output sum to 4.3e9 before the weights."""
    full = np.full((4112, 4112, 1), 255, np.uint8)
    assert np.all(one(full, (1, 1)) == 255) and np.all(one(full, (2, 3)) == 255)
    a = np.random.default_rng(41).integers(0, 256, (4112, 4112, 1), dtype=np.uint8)
    assert np.array_equal(one(a, (3, 5)), A.area_u8(a, 3, 5))
    assert np.array_equal(one(a, (1, 1)), A.area_u8(a, 1, 1))


def labels_to_mask(labels, C):
    """One-hot uint8 (h, w, C) from integer labels, -1 = no class."""
    return (labels[..., None] == np.arange(C)).astype(np.uint8)


@pytest.mark.parametrize("C", [1, 2, 15, 16])
def test_majority_is_the_restatement(C):
    rng = np.random.default_rng(C)
    h, w, H, W = 75, 270, 20, 72                                                 # a ratio of 3.75, 72 columns: two units
    coarse = rng.integers(-1, C, (9, 14))                                        # blocks of classes and of "no class"
    labels = coarse[np.sort(rng.integers(0, 9, h))][:, np.sort(rng.integers(0, 14, w))]
    exclusive = labels_to_mask(labels, C)
    overlapping = (rng.random((h, w, C)) < 0.4).astype(np.uint8)
    other_bytes = exclusive * rng.choice(np.uint8([1, 2, 7, 128, 255]), (h, w, 1))
    n0 = launches(b"area (majority)")
    for name, m in (("exclusive", exclusive), ("overlapping", overlapping), ("bytes", other_bytes), ("zero", np.zeros_like(exclusive))):
        got = one(m, (H, W), "majority")
        assert np.array_equal(got, A.majority(m, H, W)), name
        assert got.max() <= 1 and got.sum(axis=2).max() <= 1
    assert launches(b"area (majority)") == n0 + 4
    assert np.array_equal(A.majority(other_bytes, H, W), A.majority(exclusive, H, W))
    assert not one(np.zeros_like(exclusive), (H, W), "majority").any()
    if C > 1:
        assert np.array_equal(one(exclusive, (h, w), "majority"), exclusive)     # the identity keeps exclusive labels


def test_majority_ties():
    C = 4
    # 2 x 2 blocks under one output each, 70 of a kind side by side: [class, class, class, class], -1 = no class
    kinds = {(3, 3, 1, 1): 1, (1, 1, 3, 3): 1,                                   # two channels tie: the lower index
             (2, 2, -1, -1): 2,                                                  # a channel ties with "no class": the channel
             (2, -1, -1, -1): None, (0, 1, 2, -1): 0, (3, 2, -1, -1): None, (-1, -1, -1, -1): None}
    labels = np.zeros((2 * len(kinds), 140), dtype=np.int64)
    for j, b in enumerate(kinds):
        labels[2 * j:2 * j + 2] = np.tile(np.int64(b).reshape(2, 2), (1, 70))
    m = labels_to_mask(labels, C)
    got = one(m, (len(kinds), 70), "majority")
    assert np.array_equal(got, A.majority(m, len(kinds), 70))
    for j, c in enumerate(kinds.values()):
        want = np.zeros(C, np.uint8) if c is None else np.eye(C, dtype=np.uint8)[c]
        assert np.all(got[j] == want), (j, c)
    # fractional coverage: 3 -> 2, the middle pixel split in halves; class 0 | class 1 | class 1 gives 2 : 1 and 0 : 3
    m3 = labels_to_mask(np.int64([[0, 1, 1]]), 2)
    assert one(m3, (1, 2), "majority").tolist() == [[[1, 0], [0, 1]]]


# ---- the stores ------------------------------------------------------------------------------------------------------------
SCENES = [(30, 40), (20, 20)]
FINE_IMAGE = [(120, 160), (80, 80)]                                              # 4 x
FINE_MASK = [(113, 150), (75, 75)]                                               # 3.75 x, and a bit
NODATA = -32767.0


def guides(canopy=False):
    fine = {"image": [s["image"] for s in B.make_scenes(FINE_IMAGE, seed=31)],
            "mask": [s["mask"] for s in B.make_scenes(FINE_MASK, seed=32)]}
    if canopy:
        fine["canopy"] = [s["canopy"] for s in B.make_scenes([(60, 81), (20, 47)], seed=33)]
    host = {k: [(A.majority if k == "mask" else A.area_u8)(a, *s) for a, s in zip(v, SCENES)] for k, v in fine.items()}
    return fine, host


def build(lists, cls=I.InferenceScenes, **kw):
    p = {k: v for k, v in params(**kw).items() if k != "label_range" or cls is D.DeviceScenes}
    return cls(coord=None, device=DEV, **lists, **p)


def same_store(S, H):
    assert sorted(S.store) == sorted(H.store) and S.shapes == H.shapes and S.channels == H.channels
    for k in H.store:
        assert S.store[k].dtype == H.store[k].dtype and torch.equal(S.store[k].view(torch.uint8), H.store[k].view(torch.uint8)), k
    assert torch.equal(S.scene_table, H.scene_table) and [float(b) for b in S.base] == [float(b) for b in H.base]


def test_inference_store_prepare_and_predictions_are_those_of_host_resampled_rasters():
    fine, host = guides()
    lr = [s["lr_dem"] for s in B.make_scenes(SCENES, seed=30)]
    n0, m0 = launches(b"area"), launches(b"area (majority)")
    S = build(dict(lr_dem=lr, **fine), guide_resample="area")
    assert launches(b"area") == n0 + 1 and launches(b"area (majority)") == m0 + 1        # one launch per kind
    H = build(dict(lr_dem=lr, **host))
    same_store(S, H)
    assert S.guide_shapes == {"image": FINE_IMAGE, "mask": FINE_MASK} and H.guide_shapes is None
    assert [tuple(s) for s in S.shapes] == SCENES
    for i in range(2):
        a, b = I.prepare(S, [i], pad=4), I.prepare(H, [i], pad=4)
        assert a[1] == b[1] and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[0], b[0]))
    model, _ = jspsr_model()
    got, want = I.predict_scenes(model, S, batch_size=2), I.predict_scenes(model, H, batch_size=2)
    assert got.offsets == want.offsets and torch.equal(got.buffer.view(torch.int32), want.buffer.view(torch.int32))


def test_with_lr_resample_and_voids():
    fine, host = guides()
    coarse = [s["lr_dem"].copy() for s in B.make_scenes([(8, 11), (6, 6)], seed=34)]
    coarse[0][2, 3, 0], coarse[0][7, 10, 0], coarse[1][0, 0, 0] = NODATA, np.nan, NODATA
    kw = dict(lr_resample="bicubic", lr_shape=SCENES, nodata=NODATA, void_margin=1)
    S = build(dict(lr_dem=coarse, **fine), guide_resample="area", **kw)
    H = build(dict(lr_dem=coarse, **host), **kw)
    same_store(S, H)
    assert S.void_counts == H.void_counts == [2, 1] and torch.equal(S.void, H.void) and torch.equal(S.void_out, H.void_out)
    assert [tuple(s) for s in S.lr_shapes] == [(8, 11), (6, 6)]


def test_device_scenes_and_one_random_crop_batch():
    fine, host = guides(canopy=True)
    scenes = B.make_scenes(SCENES, seed=30)
    dems = {k: [s[k] for s in scenes] for k in ("lr_dem", "hr_dem")}
    S = build(dict(dems, **fine), cls=D.DeviceScenes, guide_resample="area")
    H = build(dict(dems, **host), cls=D.DeviceScenes)
    same_store(S, H)
    assert S.guide_shapes["canopy"] == [(60, 81), (20, 47)]
    batches = [next(iter(D.RandomCropBatches(st, 4, 16, rng=np.random.RandomState(5), sampler=[0, 1, 1, 0]))) for st in (S, H)]
    assert sorted(batches[0]) == sorted(batches[1])
    for k in ("lr_dem", "hr_dem", "image", "mask", "canopy", "base"):
        assert torch.equal(batches[0][k].view(torch.int32), batches[1][k].view(torch.int32)), k
    assert batches[0]["meta"] == batches[1]["meta"] and batches[0]["image"].shape == (4, 3, 16, 16)


def test_without_the_keyword_nothing_changes():
    scenes = B.make_scenes(SCENES, seed=30)
    lists = {k: [s[k] for s in scenes] for k in ("lr_dem", "image", "mask", "canopy")}
    n0 = launches(b"area") + launches(b"area (majority)")
    today, none = build(lists), build(lists, guide_resample=None)
    assert launches(b"area") + launches(b"area (majority)") == n0
    same_store(none, today)
    for k in ("image", "mask", "canopy"):
        assert np.array_equal(today.store[k].cpu().numpy(), np.concatenate([a.reshape(-1) for a in lists[k]])), k
    same_store(build(lists, guide_resample="area"), today)                       # equal shapes: the identity
    fine, _ = guides()
    with pytest.raises(ValueError, match="does not match lr_dem"):
        build(dict(lr_dem=lists["lr_dem"], **fine))
