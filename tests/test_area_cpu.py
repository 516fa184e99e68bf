"""K26 without a GPU: the integer restatement tests/area_ref.py against independent forms (exact fractions, torch's float64
average pooling), jspsr_area_axis (host code of the library) against the restatement, and the argument checks that are decided
before any launch.  Every comparison is integer equality."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import infer as I
from jspsr_amd import resample as RS
from tests import area_ref as A
from tests import batches_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = [(15, 4), (65, 64), (173, 10), (7, 1), (8, 8)]
LONG_AXES = [(65535, 1), (65535, 65534)]
ENTRIES = {"jspsr_area_axis": 5, "jspsr_area_forward": 10}


@pytest.mark.parametrize("h,H", AXES + [(64, 4)])
def test_axis_matrix_is_the_overlap_in_exact_fractions(h, H):
    m = A.axis_matrix(h, H)
    assert m.shape == (H, h) and m.dtype == np.int64
    for Y in range(H):
        lo, hi = Fraction(Y * h, H), Fraction((Y + 1) * h, H)     # the output's extent in source pixels
        for i in range(h):
            overlap = max(Fraction(0), min(hi, Fraction(i + 1)) - max(lo, Fraction(i)))
            assert overlap * H == int(m[Y, i]), (Y, i)
    assert np.array_equal(m.sum(axis=1), np.full(H, h)) and np.array_equal(m.sum(axis=0), np.full(h, H))
    assert np.max((m > 0).sum(axis=1)) <= -(-h // H) + 1


def test_area_u8_is_average_pooling_at_integer_ratios_and_the_identity():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    x = torch.from_numpy(img).permute(2, 0, 1)[None].double()
    for (H, W), k in (((16, 32), (4, 3)), ((32, 96), (2, 1)), ((8, 8), (8, 12))):
        ref = torch.floor(F.avg_pool2d(x, k) + 0.5)[0].permute(1, 2, 0).numpy().astype(np.uint8)
        assert np.array_equal(A.area_u8(img, H, W), ref), (H, W)
    assert np.array_equal(A.area_u8(img, 64, 96), img)
    one_hot = np.eye(5, dtype=np.uint8)[rng.integers(0, 5, (12, 9))]
    assert np.array_equal(A.majority(one_hot, 12, 9), one_hot)
    assert np.array_equal(A.majority(one_hot * 200, 12, 9), one_hot)            # a non-zero byte counts as 1
    halves = np.uint8([[0, 0, 0, 2], [1, 0, 0, 0], [1, 1, 0, 0], [255, 255, 255, 254]]).reshape(4, 2, 2, 1)
    assert [int(A.area_u8(b, 1, 1)[0, 0, 0]) for b in halves] == [1, 0, 1, 255]


@pytest.mark.parametrize("h,H", AXES + LONG_AXES)
def test_area_axis_is_the_restatement(h, H):
    first, count, weights = RS.area_axis(h, H)
    taps = -(-h // H) + 1
    assert first.dtype == np.int32 and count.dtype == np.int32 and weights.dtype == np.uint32
    assert first.shape == (H,) and count.shape == (H,) and weights.shape == (H, taps)
    assert count.min() >= 1 and count.max() <= taps
    # a window of one column before the first tap to one past the last possible: the weights inside are the formula's, and
    # the zeros on both sides make first and count tight (the long axes are never formed densely: 65535 x 65534 int64)
    Y = np.arange(H)[:, None]
    cols = first.astype(np.int64)[:, None] - 1 + np.arange(taps + 2)[None, :]
    ref = A.overlap(h, H, Y, cols)
    assert np.array_equal(ref[:, 1:-1], weights.astype(np.int64)) and not ref[:, 0].any()
    assert np.array_equal((ref[:, 1:] > 0).sum(axis=1), count) and np.all(ref[np.arange(H), 1] > 0)
    assert np.array_equal(weights.astype(np.int64).sum(axis=1), np.full(H, h))
    if h * H <= 1 << 20:
        m = A.axis_matrix(h, H)
        dense = np.zeros((H, h + taps), dtype=np.int64)
        dense[Y, cols[:, 1:-1]] = weights
        assert np.array_equal(dense[:, :h], m) and not dense[:, h:].any()
    assert all(not weights[Y, c:].any() for Y, c in enumerate(count))           # zero past the count
    assert RS.area_axis(h, H)[0] is first                                       # cached on the host


def test_area_axis_refusals():
    lib = _lib.load()
    first, count, weights = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros((8, 3), np.uint32)
    f, c, w = first.ctypes.data, count.ctypes.data, weights.ctypes.data
    assert lib.jspsr_area_axis(7, 8, f, c, w) == -1 and b"area_axis" in lib.jspsr_last_error()
    assert lib.jspsr_area_axis(0, 0, f, c, w) == -1 and lib.jspsr_area_axis(8, 0, f, c, w) == -1
    assert lib.jspsr_area_axis(0, 1, f, c, w) == -1 and lib.jspsr_area_axis(65536, 8, f, c, w) == -1
    assert lib.jspsr_area_axis(8, 4, None, c, w) == -1 and lib.jspsr_area_axis(8, 4, f, None, w) == -1
    assert lib.jspsr_area_axis(8, 4, f, c, None) == 0 and lib.jspsr_area_axis(8, 8, f, c, w) == 0
    with pytest.raises(ValueError, match="upsampling"):
        RS.area_axis(7, 8)
    with pytest.raises(ValueError):
        RS.area_axis(0, 1)
    with pytest.raises(ValueError):
        RS.area_axis(8, 0)
    # the K25 axis still refuses a downsampling
    with pytest.raises(ValueError, match="downsampling"):
        RS.axis_taps(8, 7)


def test_forward_refuses_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN before a launch (safe without a GPU: no device pointer is dereferenced)."""
    lib = _lib.load()
    x = 4096
    rows = np.array([[0, 8, 8, 0, 4, 4]], dtype=np.int64)

    ROWS = object()                                                             # host=ROWS: the rows below; host=None: NULL

    def call(src=x, src_numel=64, dst=x, dst_numel=16, table=x, host=ROWS, n=1, channels=3, mode=0, **row):
        r = rows.copy()
        for k, v in row.items():
            r[0, ("so", "h", "w", "do", "H", "W").index(k)] = v
        return lib.jspsr_area_forward(src, src_numel, dst, dst_numel, table, r.ctypes.data if host is ROWS else host, n, channels, mode, None)

    n0 = lib.jspsr_launch_count(b"area") + lib.jspsr_launch_count(b"area (majority)")
    for kw in (dict(src=None), dict(dst=None), dict(table=None), dict(host=None), dict(n=0), dict(n=65536), dict(channels=0), dict(channels=17),
               dict(mode=2), dict(mode=-1), dict(H=9), dict(W=9), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(src_numel=63),
               dict(dst_numel=15), dict(so=1), dict(do=1), dict(so=-1), dict(do=-1), dict(src_numel=-1),
               dict(h=65536, src_numel=65536 * 8), dict(w=65536, src_numel=65536 * 8)):
        assert call(**kw) == -1, kw
    assert b"area_forward" in lib.jspsr_last_error()
    assert call(H=9) == -1 and b"upsampling" in lib.jspsr_last_error()
    assert call(table=x + 4) == -2
    assert lib.jspsr_launch_count(b"area") + lib.jspsr_launch_count(b"area (majority)") == n0


def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert "K26 (ABI v25, additive)" in hdr and "K25 (ABI v25, additive)" in hdr
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\bint\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    assert not any(k.startswith("jspsr_area") and k.endswith("_workspace_bytes") for k in _lib.SIGNATURES)
    assert not any(hasattr(lib, name) for name in ("jspsr_area_workspace_bytes", "jspsr_area_forward_workspace_bytes"))
    assert _lib.load().jspsr_abi_version() == 25
    assert all(callable(getattr(RS, name)) for name in ("area_axis", "area_rasters", "area_resize"))
    assert os.path.exists(os.path.join(ROOT, "jspsr_amd", "csrc", "area.hip"))


def _lists(scene, fine_image, fine_mask, seed=3):
    lists = {"lr_dem": [s["lr_dem"] for s in B.make_scenes(scene, seed=seed)],
             "image": [s["image"] for s in B.make_scenes(fine_image, seed=seed + 1)],
             "mask": [s["mask"] for s in B.make_scenes(fine_mask, seed=seed + 2)]}
    return lists, {k: v for k, v in B.PARAMS.items() if k != "label_range"}


def test_store_argument_checks_need_no_gpu():
    scene = [(30, 40), (20, 20)]
    lists, p = _lists(scene, [(120, 160), (80, 80)], [(113, 150), (75, 75)])
    with pytest.raises(ValueError, match="does not match lr_dem"):              # today's behaviour without the keyword
        I.InferenceScenes(**lists, **p)
    with pytest.raises(ValueError, match="guide_resample"):
        I.InferenceScenes(**lists, guide_resample="bicubic", **p)
    small, _ = _lists(scene, [(120, 160), (80, 19)], [(113, 150), (75, 75)])
    with pytest.raises(ValueError, match="upsampling"):
        I.InferenceScenes(**small, guide_resample="area", **p)
    small, _ = _lists(scene, [(120, 160), (80, 80)], [(29, 150), (75, 75)])
    with pytest.raises(ValueError, match="upsampling of image / mask / canopy is not built"):
        I.InferenceScenes(**small, guide_resample="area", **p)
    coarse = dict(lists, lr_dem=[s["lr_dem"] for s in B.make_scenes([(8, 11), (6, 6)], seed=9)])
    with pytest.raises(ValueError, match="lr_shape"):                           # the guidance rasters fix no shape
        I.InferenceScenes(**coarse, lr_resample="bicubic", guide_resample="area", **p)
    with pytest.raises(ValueError, match="does not match"):                     # lr_resample alone still wants the scene's grid
        I.InferenceScenes(**coarse, lr_resample="bicubic", lr_shape=scene, **p)
    hr = [np.zeros((h, w, 1), np.float32) for h, w in scene]
    with pytest.raises(ValueError, match="does not match lr_dem"):
        D.DeviceScenes(hr_dem=hr, label_range=None, **lists, **p)
    with pytest.raises(ValueError, match="upsampling"):
        D.DeviceScenes(hr_dem=hr, label_range=None, guide_resample="area", **small, **p)
    with pytest.raises(ValueError, match="on the device"):
        RS.area_rasters(torch.zeros(192, dtype=torch.uint8), [(0, 8, 8)], 3, [(4, 4)])
    with pytest.raises(ValueError, match="uint8"):
        RS.area_resize(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))      # a CPU tensor
    with pytest.raises(ValueError, match="mode"):
        RS._area_mode("nearest")
