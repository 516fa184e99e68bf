"""K25 without a GPU: jspsr_resample_axis (host code of the library) against the numpy restatement tests/resample_ref.py,
the restatement against torch's float64 F.interpolate, and the argument checks that are decided before any launch.

Bounds.  The taps are compared bit for bit: integers, and doubles rounded once.  The restatement against float64 torch:
|out - ref| <= 2^-23 |ref| + 12 * 2^-24 * sum |w_ij| |v_ij - c| (resample_ref.tolerance): the last rounding, and the twelve
roundings of the longest path before it, each relative to a term of that sum."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import infer as I
from jspsr_amd import resample as RS
from tests import batches_ref as B
from tests import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = [(1, 5), (2, 7), (5, 19), (16, 60), (35, 130), (89, 334), (7, 7), (3, 12)]
SHAPES = [((1, 1), (5, 3)), ((2, 3), (7, 5)), ((5, 4), (19, 15)), ((16, 16), (60, 60)), ((35, 19), (130, 70)),
          ((89, 89), (334, 334)), ((7, 7), (7, 7)), ((3, 8), (12, 8))]
MODES = ("bicubic", "bilinear")
ENTRIES = {"jspsr_resample_axis": 5, "jspsr_resample_forward": 15}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,H", AXES)
def test_axis_taps_are_the_restatements_bit_for_bit(h, H, mode):
    first, weights = RS.axis_taps(h, H, mode)
    rf, rw = R.axis_taps(h, H, mode)
    assert first.dtype == np.int32 and weights.dtype == np.float32 and first.shape == (H,) and weights.shape == (H, 4)
    assert np.array_equal(first, rf) and np.array_equal(bits(weights), bits(rw))
    # every row sums to 1 within 2 ulp
    assert np.all(np.abs(weights.astype(np.float64).sum(axis=1) - 1.0) <= 2 * 2.0 ** -23)
    nt, ct = R.NT[mode], R.CENTRE[mode]
    assert first.min() >= -1 - ct and first.max() + ct <= h - 1                # pixel i is -1 (above the first row) .. h - 1
    taps = np.clip(first[:, None].astype(np.int64) + np.arange(nt), 0, h - 1)
    assert taps.min() >= 0 and taps.max() <= h - 1
    assert np.all(np.diff(first) >= 0) and np.all(np.diff(first) <= 1)         # what the kernel's patch size rests on
    if mode == "bilinear":
        assert not weights[:, 2:].any()
    if h == H:
        assert np.array_equal(weights, np.tile(np.float32([0, 1, 0, 0] if mode == "bicubic" else [1, 0, 0, 0]), (H, 1)))
        assert np.array_equal(first + ct, np.arange(H))
    assert RS.axis_taps(h, H, mode)[0] is first                                # cached on the host


def test_downsampling_and_bad_arguments_are_refused():
    lib = _lib.load()
    first, weights = np.zeros(8, np.int32), np.zeros((8, 4), np.float32)
    f, w = first.ctypes.data, weights.ctypes.data
    assert lib.jspsr_resample_axis(8, 7, 0, f, w) == -1 and b"resample_axis" in lib.jspsr_last_error()
    assert lib.jspsr_resample_axis(0, 4, 0, f, w) == -1 and lib.jspsr_resample_axis(4, 8, 2, f, w) == -1
    assert lib.jspsr_resample_axis(4, 8, 0, None, w) == -1 and lib.jspsr_resample_axis(4, 8, 1, f, None) == -1
    assert lib.jspsr_resample_axis(4, 8, 0, f, w) == 0
    for bad in ((8, 7, "bicubic"), (3, 2, "bilinear")):
        with pytest.raises(ValueError, match="downsampling"):
            RS.axis_taps(*bad)
    with pytest.raises(ValueError):
        RS.axis_taps(4, 8, "nearest")
    with pytest.raises(ValueError):
        RS.axis_taps(0, 8)


def test_forward_refuses_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN before a launch (safe without a GPU: no device pointer is dereferenced)."""
    lib = _lib.load()
    x = 4096
    rows = np.array([[0, 4, 4, 0, 8, 8, 0, 0]], dtype=np.int64)

    def call(src=x, src_numel=16, dst=x, dst_numel=64, table=x, host=None, n=1, first=x, weights=x, n_taps=8, mode=0, clamp=None,
             sv=None, dv=None, **row):
        r = rows.copy()
        for k, v in row.items():
            r[0, ("so", "h", "w", "do", "H", "W", "yt", "xt").index(k)] = v
        return lib.jspsr_resample_forward(src, src_numel, dst, dst_numel, table, r.ctypes.data if host is None else host, n, first, weights,
                                          n_taps, mode, clamp, sv, dv, None)

    n0 = lib.jspsr_launch_count(b"resample") + lib.jspsr_launch_count(b"resample (void)")
    for kw in (dict(src=None), dict(dst=None), dict(table=None), dict(first=None), dict(weights=None), dict(n=0), dict(n=65536),
               dict(mode=2), dict(sv=x), dict(dv=x), dict(H=3), dict(W=3), dict(h=0), dict(src_numel=15), dict(dst_numel=63),
               dict(so=1), dict(do=1), dict(so=-1), dict(do=-1), dict(n_taps=7), dict(yt=1), dict(xt=-1)):
        assert call(**kw) == -1, kw
    assert b"resample_forward" in lib.jspsr_last_error()
    for kw in (dict(src=x + 2), dict(dst=x + 1), dict(first=x + 2), dict(weights=x + 3), dict(clamp=x + 2), dict(table=x + 4)):
        assert call(**kw) == -2, kw
    assert lib.jspsr_launch_count(b"resample") + lib.jspsr_launch_count(b"resample (void)") == n0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src,dst", SHAPES)
def test_restatement_is_torch_in_float64_within_its_roundings(src, dst, mode):
    a = R.terrain(np.random.default_rng(src[0] * 1000 + dst[1]), *src)
    out = R.resample(a, *dst, mode)
    ref = R.torch_ref(a, *dst, mode)
    tol = R.tolerance(ref, a, *dst, mode)
    err = np.abs(out.astype(np.float64) - ref)
    print(f"{src} -> {dst} {mode}: max err {err.max():.3e}, max err / tol {np.max(err / tol):.3f}")
    assert out.dtype == np.float32 and out.shape == dst and np.all(err <= tol)
    if src == dst:
        assert np.array_equal(bits(out), bits(a))


def test_restatement_clamp_and_void_rule():
    a = np.zeros((6, 6), np.float32)
    a[:, 3:] = 1000
    free, held = R.resample(a, 23, 23), R.resample(a, 23, 23, clamp=(0, 1000))
    assert free.min() < 0 and free.max() > 1000 and held.min() == 0 and held.max() == 1000
    assert np.array_equal(held, np.clip(free, 0, 1000))
    a[2, 2] = np.nan
    assert np.isnan(R.resample(a, 23, 23, clamp=(0, 1000))).any()               # the clamp keeps a NaN
    v = np.zeros((6, 6), np.uint8)
    v[2, 2] = 1
    fine = R.void_plane(v, 23, 23)
    yy = np.clip(np.floor((np.arange(23) + 0.5) * 6 / 23 - 0.5), 0, 5).astype(int)   # the centre tap: the coordinate's floor
    assert np.array_equal(fine, v[yy][:, yy]) and fine.sum() > 1


def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert "K25 (ABI v25, additive)" in hdr
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\bint\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    assert not any(k.startswith("jspsr_resample") and k.endswith("_workspace_bytes") for k in _lib.SIGNATURES)
    assert _lib.load().jspsr_abi_version() == 25
    assert all(callable(getattr(RS, name)) for name in ("axis_taps", "resample_rasters", "resize"))
    assert os.path.exists(os.path.join(ROOT, "jspsr_amd", "csrc", "resample.hip"))
    assert "bicubic resize" not in open(os.path.join(ROOT, "jspsr_amd", "evaluate.py")).read().split('"""')[1]


def _lists(fine, coarse, seed=3):
    scenes = B.make_scenes(fine, seed=seed)
    small = B.make_scenes(coarse, seed=seed + 1)
    lists = {k: [s[k] for s in scenes] for k in ("image", "mask")}
    lists["lr_dem"] = [s["lr_dem"] for s in small]
    return lists, {k: v for k, v in B.PARAMS.items() if k != "label_range"}


def test_store_argument_checks_need_no_gpu():
    lists, p = _lists([(30, 40), (20, 20)], [(8, 11), (6, 6)])
    with pytest.raises(ValueError, match="does not match lr_dem"):              # today's behaviour without the keyword
        I.InferenceScenes(**lists, **p)
    with pytest.raises(ValueError, match="mode"):
        I.InferenceScenes(**lists, lr_resample="nearest", **p)
    with pytest.raises(ValueError, match="lr_shape"):                           # nothing to take the shapes from
        I.InferenceScenes(lr_dem=lists["lr_dem"], lr_resample="bicubic", **p)
    with pytest.raises(ValueError, match="lr_shape"):
        I.InferenceScenes(**lists, lr_resample="bicubic", lr_shape=(30, 41), **p)
    with pytest.raises(ValueError, match="lr_shape"):                           # only together with lr_resample
        I.InferenceScenes(lr_dem=lists["lr_dem"], lr_shape=(30, 40), **p)
    big, _ = _lists([(30, 40), (20, 20)], [(8, 11), (21, 6)])
    with pytest.raises(ValueError, match="downsampling"):
        I.InferenceScenes(**big, lr_resample="bicubic", **p)
    hr = [np.zeros((30, 40, 1), np.float32), np.zeros((20, 20, 1), np.float32)]
    with pytest.raises(ValueError, match="does not match lr_dem"):
        D.DeviceScenes(hr_dem=hr, label_range=None, **lists, **p)
    from jspsr_amd import evaluate as EV
    with pytest.raises(ValueError, match="resize_input"):
        EV.evaluate(torch.nn.Identity(), [], None, None, "JSPSR", {}, resize_input="bilinear")
    with pytest.raises(ValueError, match="fp32"):
        RS.resize(torch.zeros(1, 1, 4, 4), (8, 8))                              # a CPU tensor
    with pytest.raises(ValueError, match="on the device"):
        RS.resample_rasters(torch.zeros(16), [(0, 4, 4)], [(8, 8)])
