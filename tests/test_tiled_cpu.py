"""Tiled whole-scene inference (K15) without a GPU: the cover planner of `jspsr_amd.cover` against its properties, against
`tiles._weight_1d` / `tiles.merge_tiles` on the reference's own covers and against the independent restatement in
tests/tiled_ref.py; the argument errors of the Python surface; the two entry points in the header, the built library and the
binding.  Weights and merges are compared with ==."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import infer as I
from jspsr_amd import tiles as T
from jspsr_amd.cover import axis_cover, plan_cover
from tests import tiled_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("jspsr_scene_prepare_windows", "jspsr_scene_merge_windows")


def draws(n, seed=15):
    """(L, k, overlap, trim) with 2 * trim <= overlap < k, trim <= k / 4 and L >= k; every tenth draw has L == k."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        k = int(rs.randint(2, 97))
        trim = int(rs.randint(0, k // 4 + 1))
        if 2 * trim >= k:
            continue
        overlap = int(rs.randint(2 * trim, k))
        L = k if len(out) % 10 == 0 else k + int(rs.randint(1, 6 * k))
        out.append((L, k, overlap, trim))
    return out


def test_planner_properties_over_a_seeded_sweep():
    seen_clip = seen_hard = 0
    for L, k, overlap, trim in draws(1500):
        o, w, lo = axis_cover(L, k, overlap, trim)
        where = (L, k, overlap, trim)
        n = len(o)
        assert o.dtype == np.int32 and w.dtype == np.float32 and lo.dtype == np.int32 and w.shape == (n, k) and lo.shape == (L,)
        assert o[0] == 0 and o[-1] + k == L, where
        assert n == 1 or (np.diff(o) > 0).all() and (o[:-1] + k - o[1:] >= overlap).all(), where
        full = np.zeros((n, L), np.float32)                                     # all non-zero weights lie inside their tile
        for i in range(n):
            full[i, o[i]:o[i] + k] = w[i]
        live = full != 0
        count = live.sum(0)
        assert ((count == 1) | (count == 2)).all(), where
        first = live.argmax(0)
        assert np.array_equal(first.astype(np.int32), lo), where
        two = count == 2
        assert live[np.minimum(first + 1, n - 1), np.arange(L)][two].all(), where       # the second one is the neighbour
        total = full.astype(np.float64).sum(0)
        assert np.abs(total - 1).max() <= 2.0 ** -24, (where, np.abs(total - 1).max())
        if trim:                                                                # trimmed margins carry no weight; the scene's edge does
            assert not w[1:, :trim].any() and not w[:-1, k - trim:].any(), where
            assert w[0, 0] == 1 and w[-1, -1] == 1, where
        ro, rw, rlo = R.axis(L, k, overlap, trim)                               # the independent restatement
        assert list(o) == ro and np.array_equal(w, rw) and np.array_equal(lo, rlo), where
        seen_clip += n > 2 and bool((o[2:] + trim < o[:-2] + k - trim).any())
        seen_hard += n > 1 and bool((o[:-1] + k - o[1:] == 2 * trim).any())
    assert seen_clip > 20 and seen_hard > 0                                     # the seam clip and the zero-width seam were drawn


def test_seam_clip_example():
    """L = 61, k = 32, overlap 4: origins 0, 14, 29 -- tile 2 starts inside tile 0 and has weight 0 before tile 0 ends."""
    o, w, lo = axis_cover(61, 32, 4, 0)
    assert list(o) == [0, 14, 29]
    assert not w[2, :3].any() and w[2, 3] != 0 and w[0, -1] != 0
    assert list(lo[29:33]) == [0, 0, 0, 1]
    o, w, lo = axis_cover(57, 32, 4, 0)                                          # two tiles sharing 7 pixels
    assert list(o) == [0, 25] and np.array_equal(w[0, 25:], np.linspace(1, 0, 9)[1:-1].astype(np.float32))


@pytest.mark.parametrize("L,k,overlap,n_x", [(334, 128, 25, 3), (231, 128, 25, 2)])
def test_reference_covers_equal_the_reference_tables(L, k, overlap, n_x):
    o, w, lo = axis_cover(L, k, overlap, 0)
    stride, n = T.get_tile(L, k)
    assert n == n_x * n_x and list(o) == [stride * i for i in range(n_x)]
    if L == 334:
        assert list(o) == [0, 103, 206]
    for pos in range(n_x):
        want = T._weight_1d(k, stride, n_x, pos, "cpu", torch.float32).numpy()
        assert np.array_equal(w[pos], want), pos
    # the merge: tiled_ref on this cover == tiles.merge_tiles' CPU path at border 0, bit for bit
    rs = np.random.RandomState(L)
    tiles = rs.uniform(100, 900, (n, 1, k, k)).astype(np.float32)
    want = T.merge_tiles(torch.from_numpy(tiles), L, 0.0).numpy()
    c = plan_cover(L, L, k, overlap)
    assert (c.n_y, c.n_x, c.n) == (n_x, n_x, n) and c.windows()[1] == (0, stride)
    got = R.merge(tiles[:, 0], c._asdict())
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(R.merge(tiles[:, 0], R.cover(L, L, k, overlap)), want)


def test_rectangular_cover_and_single_tile_axis():
    c = plan_cover(64, 120, (24, 40), 10)
    assert (c.kh, c.kw) == (24, 40) and c.wy.shape == (c.n_y, 24) and c.wx.shape == (c.n_x, 40)
    assert c.oy[-1] + 24 == 64 and c.ox[-1] + 40 == 120 and c.lo_y.shape == (64,) and c.lo_x.shape == (120,)
    assert c.windows() == [(int(y), int(x)) for y in c.oy for x in c.ox]
    one = plan_cover(32, 91, 32, 8, 2)
    assert one.n_y == 1 and (one.wy == 1).all() and not one.lo_y.any() and one.n_x > 1
    r = R.cover(64, 120, (24, 40), 10)
    assert all(np.array_equal(getattr(c, f), r[f]) for f in ("oy", "ox", "wy", "wx", "lo_y", "lo_x"))


def test_a_nan_in_a_trimmed_margin_is_dropped_by_the_reference_merge():
    c = R.cover(70, 91, 32, 8, 2)
    rs = np.random.RandomState(3)
    m = rs.uniform(0, 1, (len(c["oy"]) * len(c["ox"]), 32, 32)).astype(np.float32)
    clean = R.merge(m, c)
    for ty in range(len(c["oy"])):
        for tx in range(len(c["ox"])):
            dead = (c["wy"][ty][:, None] == 0) | (c["wx"][tx][None, :] == 0)
            m[ty * len(c["ox"]) + tx][dead] = np.nan
    assert np.isnan(m).any() and np.array_equal(R.merge(m, c), clean)


def test_planner_errors():
    with pytest.raises(ValueError, match="twice the trim"):
        plan_cover(100, 100, 32, 6, 4)
    with pytest.raises(ValueError, match="not below the tile side"):
        plan_cover(100, 100, 32, 32)
    with pytest.raises(ValueError, match="not below the tile side"):
        plan_cover(100, 100, (32, 16), 16)
    with pytest.raises(ValueError, match="rectangular"):
        plan_cover(20, 100, 32, 8)
    assert plan_cover(100, 100, 32, 8, 4).trim == 4                              # overlap == 2 * trim is allowed


class _Store:
    """What predict_scenes reads of a store before its first launch."""
    device = "cpu"
    channels = {"lr_dem": 1, "image": 3}

    def __init__(self, shapes):
        self.shapes = shapes
        self.ids = [str(i) for i in range(len(shapes))]

    def __len__(self):
        return len(self.shapes)


def test_predict_scenes_argument_errors():
    model = types.SimpleNamespace(name="jspsr", size_multiple=8, eval=lambda: None)
    big = _Store([(100, 100)])
    with pytest.raises(NotImplementedError, match="tile together with tta"):
        I.predict_scenes(model, big, tile=32, tta="d4")
    with pytest.raises(ValueError, match="multiple of the model's 8"):
        I.predict_scenes(model, big, tile=36)
    with pytest.raises(ValueError, match="multiple of the model's 8"):
        I.predict_scenes(model, big, tile=(32, 36))
    with pytest.raises(ValueError, match="rectangular"):
        I.predict_scenes(model, _Store([(100, 100), (20, 100)]), tile=32)
    with pytest.raises(ValueError, match="pad must be 0"):
        I.predict_scenes(model, big, tile=32, pad=4)
    with pytest.raises(ValueError, match="pad must be 0"):
        I.predict_scenes(model, big, tile=32, pad="pow2")
    with pytest.raises(ValueError, match="twice the trim"):
        I.predict_scenes(model, big, tile=32, overlap=6, trim=4)
    with pytest.raises(ValueError, match="not below the tile side"):
        I.predict_scenes(model, big, tile=32, overlap=32)
    with pytest.raises(ValueError, match="tile"):
        I.predict_scenes(model, big, tile=(32, 32, 32))
    with pytest.raises(ValueError, match="twice the trim"):                     # the default overlap, a quarter of the smaller side
        I.predict_scenes(model, big, tile=(32, 64), trim=5)


def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name         # one binding argument per parameter
    lib.jspsr_abi_version.restype = ctypes.c_int
    assert lib.jspsr_abi_version() == 25 == _lib.load().jspsr_abi_version()
    assert "K15 (ABI v25)" in hdr and "is NOT read" in hdr


def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN with a message, before a launch (safe without a GPU: no pointer is dereferenced on the
    device, the host arrays are real)."""
    lib = _lib.load()
    x = ctypes.c_void_p(4096)

    def message():
        return lib.jspsr_last_error().decode()

    six_p, six_ll, six_i = ctypes.c_void_p * 6, ctypes.c_longlong * 6, ctypes.c_int * 6
    src, nbytes, out = six_p(), six_ll(), six_p()
    ch, coff, pitch = six_i(), six_i(), six_i()

    def prepare(B=2, kh=24, kw=16, samples=x, scenes=x, mask_div=3, flags=0):
        return lib.jspsr_scene_prepare_windows(src, nbytes, out, ch, coff, pitch, scenes, 1, samples, B, kh, kw, flags, -80.0, 933.0,
                                               mask_div, None)

    out[5], ch[5], pitch[5] = 4096, 2, 2                                        # coord alone: no store needed
    assert prepare(B=0) == -1 and "scene_prepare_windows" in message()
    assert prepare(kw=0) == -1 and prepare(kh=0) == -1 and prepare(samples=None) == -1 and prepare(scenes=None) == -1
    assert prepare(mask_div=0) == -1 and prepare(flags=64) == -1
    assert lib.jspsr_scene_prepare_windows(None, nbytes, out, ch, coff, pitch, x, 1, x, 2, 24, 16, 0, -80.0, 933.0, 3, None) == -1
    assert prepare(samples=ctypes.c_void_p(4098)) == -2 and "aligned" in message()
    out[5] = None
    assert prepare() == -1 and "no output" in message()
    out[1], ch[1], pitch[1] = 4096, 1, 1
    assert prepare() == -1 and "hr_dem" in message()
    out[1] = None
    out[3], ch[3], pitch[3] = 4096, 2, 2
    assert prepare() == -1 and "store" in message()
    out[3], ch[3], pitch[3] = 4098, 2, 2
    assert prepare() == -2

    def merge(dtype=0, tiles=x, wy=x, lo_x=x, ox=x, samples=x, out=x, S=2, n_y=3, n_x=4, kh=32, kw=32, H=70, W=91):
        return lib.jspsr_scene_merge_windows(dtype, tiles, wy, x, x, lo_x, x, ox, samples, out, S, n_y, n_x, kh, kw, H, W, 1, 1, -80.0,
                                             933.0, None)

    assert merge(S=0) == -1 and "scene_merge_windows" in message()
    assert merge(kw=0) == -1 and merge(kh=0) == -1 and merge(H=0) == -1 and merge(n_x=0) == -1
    for name in ("tiles", "wy", "lo_x", "ox", "samples", "out"):
        assert merge(**{name: None}) == -1, name
    assert merge(dtype=2) == -1
    assert merge(n_x=2) == -1 and "do not cover" in message()                   # 2 x 32 < 91
    assert merge(kh=80) == -1 and "do not cover" in message()                   # a tile taller than the scene
    assert merge(tiles=ctypes.c_void_p(4098)) == -2 and "aligned" in message()
    assert merge(tiles=ctypes.c_void_p(4097), dtype=1) == -2                    # bf16 tiles need 2-byte alignment only
    assert merge(out=ctypes.c_void_p(4098)) == -2 and merge(wy=ctypes.c_void_p(4097)) == -2
