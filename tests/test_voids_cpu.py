"""Voids in whole-scene inference (K17) without a GPU: the brute-force rule of tests/voids_ref.py against the two-phase
scheme the kernels run and against scipy's exact EDT; void detection, the base and the range checks over valid pixels and the
refusals of `InferenceScenes(nodata=...)`; the new entries in the header, the built library and the binding; their argument
errors before any launch.  Everything is compared with ==."""
import ctypes
import os
import re

import numpy as np
import pytest

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import infer as I
from tests import voids_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"jspsr_scene_nearest_seed_workspace_bytes": 1, "jspsr_scene_nearest_seed": 10, "jspsr_scene_fill_voids": 8,
           "jspsr_scene_mask_out": 8}
P = dict(elev_min=-80, elev_max=933, elev_log=True)


def masks():
    rs = np.random.RandomState(17)
    out = []
    for h, w in ((1, 1), (1, 7), (7, 1), (5, 9), (13, 17), (24, 40)):
        out.append((f"{h}x{w} random", rs.rand(h, w) < 0.3))
        out.append((f"{h}x{w} empty", np.zeros((h, w), bool)))
        sparse = np.zeros((h, w), bool)
        sparse[rs.randint(h), rs.randint(w)] = True
        sparse[rs.randint(h), rs.randint(w)] = True
        out.append((f"{h}x{w} sparse", sparse))
    yy, xx = np.mgrid[0:16, 0:16]
    out.append(("16x16 checkerboard", (yy + xx) % 2 == 0))
    return out


@pytest.mark.parametrize("name,seed", masks(), ids=[n for n, _ in masks()])
def test_brute_force_rule_is_the_two_phase_scheme(name, seed):
    for limit in (None, 3, 1):
        src, d2 = R.nearest_seed_ref(seed, limit)
        s2, e2 = R.two_phase(seed, limit)
        assert np.array_equal(src, s2) and np.array_equal(d2, e2), (name, limit)
    src, d2 = R.nearest_seed_ref(seed)
    H, W = seed.shape
    if seed.any():
        assert (src >= 0).all() and seed.reshape(-1)[src].all()
        sy, sx = src // W, src % W
        yy, xx = np.mgrid[0:H, 0:W]
        assert np.array_equal((sy - yy) ** 2 + (sx - xx) ** 2, d2)
        assert np.array_equal(src[seed], (yy * W + xx)[seed]) and not d2[seed].any()     # a seed finds itself
        assert np.array_equal(d2, R.d2_min_ref(seed))
        s3, e3 = R.nearest_seed_ref(seed, 3)
        far = d2 > 9
        assert (s3[far] == -1).all() and (e3[far] == -1).all()
        assert np.array_equal(s3[~far], src[~far]) and np.array_equal(e3[~far], d2[~far])
    else:
        assert (src == -1).all() and (d2 == -1).all()


def test_ties_go_by_abs_dx_then_dx_then_dy():
    seed = np.zeros((5, 5), bool)
    seed[0, 2] = seed[4, 2] = seed[2, 0] = seed[2, 4] = True                    # four seeds at distance 2 of the centre
    src, d2 = R.nearest_seed_ref(seed)
    assert d2[2, 2] == 4 and src[2, 2] == 0 * 5 + 2                             # |dx| = 0 first, then the upper one
    seed[0, 2] = seed[4, 2] = False
    assert R.nearest_seed_ref(seed)[0][2, 2] == 2 * 5 + 0                       # then the left one
    assert R.two_phase(seed)[0][2, 2] == 2 * 5 + 0


@pytest.mark.parametrize("density", [0.5, 0.01])
def test_d2_is_scipys_exact_edt(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    seed = np.random.RandomState(int(density * 100)).rand(200, 300) < density
    want = np.rint(ndimage.distance_transform_edt(~seed) ** 2).astype(np.int64)
    assert np.array_equal(R.d2_min_ref(seed), want)
    sub = seed[:40, :60]                                                        # and the whole rule on a corner of it
    src, d2 = R.two_phase(sub)
    assert np.array_equal(d2, np.rint(ndimage.distance_transform_edt(~sub) ** 2).astype(np.int32))
    assert np.array_equal(src, R.nearest_seed_ref(sub)[0])


def test_void_detection():
    a = np.array([[1.0, -32767.0, np.nan], [np.inf, -np.inf, 0.0]], dtype=np.float32)
    assert D.void_pixels(a, -32767).tolist() == [[False, True, True], [True, True, False]]
    assert D.void_pixels(a, float("nan")).tolist() == [[False, False, True], [True, True, False]]
    assert D.void_pixels(a, -99999.0).tolist() == [[False, False, True], [True, True, False]]
    assert D.void_pixels(a, 0).tolist() == [[False, False, True], [True, True, True]]
    assert D.void_pixels(a, np.float64(-32767.0000001)).tolist()[0][1]          # compared as np.float32(nodata)
    assert np.array_equal(D.void_pixels(a, -32767), R.void_pixels(a, -32767))


def dem(h, w, seed=3):
    rs = np.random.RandomState(seed)
    return (200 + rs.uniform(0, 300, (h, w, 1))).astype(np.float32)


def test_base_and_range_checks_read_valid_pixels_only(monkeypatch):
    seen = {}
    monkeypatch.setattr(D.DeviceScenes, "_fill_voids", lambda self, voids, *a: seen.update(voids=voids, args=a))
    a, b = dem(6, 8), dem(5, 5, seed=4)
    a[0, 0] = -32767
    a[3, 4] = np.nan
    b[4, 4] = np.inf
    with pytest.raises(AssertionError):                                         # today: the void fails the range checks
        I.InferenceScenes([a, b], relative=True, device="cpu", **P)
    S = I.InferenceScenes([a, b], relative=True, device="cpu", nodata=-32767, void_margin=2, fill_limit=7, **P)
    va, vb = R.void_pixels(a, -32767), R.void_pixels(b, -32767)
    assert S.base == [np.min(a[~va]), np.min(b[~vb])] and all(np.isfinite(S.base))
    assert np.array_equal(seen["voids"][0], va) and np.array_equal(seen["voids"][1], vb) and seen["args"] == (-32767, 2, 7)
    assert I.InferenceScenes([a, b], relative=False, device="cpu", nodata=-32767, **P).base == [0, 0]
    assert I.InferenceScenes([a, b], relative=True, device="cpu", nodata=-32767, base=[5.0, 6.0], **P).base == [5.0, 6.0]
    bad = a.copy()
    bad[2, 2] = 5000.0                                                          # a valid pixel out of range is still refused
    with pytest.raises(AssertionError, match="not within"):
        I.InferenceScenes([bad], relative=True, device="cpu", nodata=-32767, **P)
    low = a.copy()
    low[2, 2] = -80.5                                                           # the log domain, over the valid pixels
    with pytest.raises(AssertionError, match="elev_min"):
        I.InferenceScenes([low], relative=False, device="cpu", nodata=-32767, **P)
    with pytest.raises(AssertionError):                                         # -32767 is a value like any other under nodata=NaN
        I.InferenceScenes([a], relative=True, device="cpu", nodata=float("nan"), **P)


def test_refusals():
    a = dem(4, 4)
    gone = np.full((3, 3, 1), -32767, dtype=np.float32)
    gone[1, 1] = np.nan
    with pytest.raises(ValueError, match="scene second.*no valid pixel"):
        I.InferenceScenes([a, gone], ids=["first", "second"], device="cpu", nodata=-32767, **P)
    for name in ("void_margin", "fill_limit"):
        for bad in (-1, 1.5, "2", True):
            with pytest.raises(ValueError, match=name):
                I.InferenceScenes([a], device="cpu", nodata=-32767, **{name: bad}, **P)
    with pytest.raises(ValueError, match="void_margin"):
        I.InferenceScenes([a], device="cpu", void_margin=None, **P)
    with pytest.raises(NotImplementedError, match="hr_dem"):
        D.DeviceScenes([a], [a], device="cpu", nodata=-32767, **P)
    with pytest.raises(ValueError, match="limit"):
        I.nearest_seed(None, [(3, 3)], limit=-1)
    with pytest.raises(ValueError, match="shapes"):
        I.nearest_seed(None, [])


def test_nodata_none_adds_nothing_and_a_store_without_voids_launches_nothing():
    a = dem(6, 8)
    S = I.InferenceScenes([a], relative=True, device="cpu", **P)
    assert not {"void", "void_out", "void_counts", "nodata"} & set(S.__dict__)
    assert S.void is None and S.void_out is None and S.void_counts is None and S.nodata is None
    with pytest.raises(ValueError, match="without nodata"):
        S.void_mask(0)
    T = I.InferenceScenes([a, a[:3]], relative=True, device="cpu", nodata=-32767, void_margin=3, **P)      # no void in it
    assert T.void_counts == [0, 0] and T.void.dtype.is_floating_point is False and T.void.numel() == 48 + 24
    assert T.void_out is T.void and not bool(T.void.any()) and T.nodata == -32767
    assert T.void_mask(1).shape == (3, 8) and T.void_mask(1, out=True).dtype.is_floating_point is False
    assert np.array_equal(T.store["lr_dem"].numpy(), np.concatenate([a.reshape(-1), a[:3].reshape(-1)]))
    assert T.base == [np.min(a), np.min(a[:3])]


def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert "K17 (ABI v25, additive)" in hdr
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\b(?:int|size_t)\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    lib.jspsr_abi_version.restype = ctypes.c_int
    assert lib.jspsr_abi_version() == 25 == _lib.load().jspsr_abi_version()
    assert all(callable(getattr(I, name)) for name in ("nearest_seed", "fill_voids", "mask_out"))
    assert os.path.exists(os.path.join(ROOT, "jspsr_amd", "csrc", "scene_voids.hip"))


def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN with a message that names the entry, before a launch (safe without a GPU: no device
    pointer is dereferenced, the host table is real)."""
    lib = _lib.load()
    x, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    counts = {n: lib.jspsr_launch_count(n) for n in (b"scene_nearest_seed", b"scene_fill_voids", b"scene_mask_out")}

    def message():
        return lib.jspsr_last_error().decode()

    def table(*rows):
        return np.ascontiguousarray(rows, dtype=np.int64)

    good = table((0, 5, 9), (45, 3, 3))

    def nearest(seed=x, pixels=54, scenes=x, host=good, n=2, limit=0, src=x, d2=x, work=x):
        return lib.jspsr_scene_nearest_seed(seed, pixels, scenes, None if host is None else host.ctypes.data, n, limit, src, d2,
                                            work, None)

    for kw in (dict(seed=None), dict(scenes=None), dict(host=None), dict(src=None), dict(d2=None), dict(work=None), dict(pixels=0),
               dict(n=0), dict(n=-1)):
        assert nearest(**kw) == -1 and "scene_nearest_seed" in message(), kw
    assert nearest(limit=-1) == -1 and "negative limit" in message()
    assert nearest(host=table((0, 32768, 1)), n=1, pixels=32768) == -1 and "32767" in message()
    assert nearest(host=table((0, 1, 40000)), n=1, pixels=40000) == -1 and "32767" in message()
    assert nearest(pixels=53) == -1 and "leaves the plane" in message()
    assert nearest(host=table((-1, 5, 9)), n=1) == -1 and "leaves the plane" in message()
    assert nearest(host=table((0, 0, 9)), n=1) == -1 and "leaves the plane" in message()
    assert nearest(src=odd) == -2 and "aligned" in message()
    assert nearest(d2=odd) == -2 and nearest(scenes=ctypes.c_void_p(4100)) == -2 and nearest(work=ctypes.c_void_p(4097)) == -2
    lib_ws = lib.jspsr_scene_nearest_seed_workspace_bytes
    assert lib_ws(0) == 0 and lib_ws(-5) == 0 and lib_ws(1) == 16 and lib_ws(4096 * 4096) == 2 * 4096 * 4096

    def fill(dem=x, void=x, src=x, pixels=54, scenes=x, n=2, base=x):
        return lib.jspsr_scene_fill_voids(dem, void, src, pixels, scenes, n, base, None)

    for kw in (dict(dem=None), dict(void=None), dict(scenes=None), dict(base=None), dict(pixels=0), dict(n=0)):
        assert fill(**kw) == -1 and "scene_fill_voids" in message(), kw
    for kw in (dict(dem=odd), dict(src=odd), dict(base=odd), dict(scenes=ctypes.c_void_p(4100))):
        assert fill(**kw) == -2 and "aligned" in message(), kw

    def mask(out=x, out_len=54, plane=x, pixels=54, rows=x, m=2, nodata=-32767.0):
        return lib.jspsr_scene_mask_out(out, out_len, plane, pixels, rows, m, nodata, None)

    for kw in (dict(out=None), dict(plane=None), dict(rows=None), dict(out_len=0), dict(pixels=-3), dict(m=0)):
        assert mask(**kw) == -1 and "scene_mask_out" in message(), kw
    for kw in (dict(out=odd), dict(rows=ctypes.c_void_p(4100))):
        assert mask(**kw) == -2 and "aligned" in message(), kw
    assert counts == {n: lib.jspsr_launch_count(n) for n in counts}
