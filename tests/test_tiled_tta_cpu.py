"""The tiled self-ensemble (K16) without a GPU: the numpy restatement of tests/tiled_tta_ref.py against `infer.d4_apply` /
`d4_invert`; the new entry point in the header, the built library and the binding; its refusals before any launch; the
argument errors of `predict_scenes(window_tta=...)`.  Everything is compared with ==."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from jspsr_amd import _lib
from jspsr_amd import infer as I
from tests import tiled_tta_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "jspsr_scene_prepare_windows_d4"


def test_index_map_is_d4_apply_for_all_sixteen_codes():
    m = np.arange(35, dtype=np.float32).reshape(5, 7) + 1                       # distinct values
    for code in range(16):
        t = I.d4_apply(m, code)
        assert t.shape == ((7, 5) if code & 4 else (5, 7)), code
        for i in range(t.shape[0]):
            for j in range(t.shape[1]):
                sy, sx = R.d4_source(code, 5, 7, i, j)
                assert 0 <= sy < 5 and 0 <= sx < 7 and t[i, j] == m[sy, sx], (code, i, j)
        assert np.array_equal(R.window_transform(m[None], code)[0], t)
        assert np.array_equal(R.carried_back(t[None], code)[0], m)
        assert np.array_equal(I.d4_apply(m, I.d4_canonical(code)), t)           # 16 codes, 8 elements


def test_mean_tiles_is_a_sequential_fp32_sum_and_one_division():
    rs = np.random.RandomState(16)
    tiles = [rs.uniform(-0.2, 1.2, (3, 6, 10)).astype(np.float32) for _ in range(8)]
    for K in (1, 2, 3, 8):
        got = R.mean_tiles(tiles[:K])
        acc = tiles[0].copy()
        for y in tiles[1:K]:
            acc = acc + y
            assert acc.dtype == np.float32
        assert got.dtype == np.float32 and np.array_equal(got, acc / np.float32(K))
    assert np.array_equal(R.mean_tiles(tiles[:1]), tiles[0])                    # K = 1: x / 1 is x
    assert not np.array_equal(R.mean_tiles(tiles[:3]), R.mean_tiles(tiles[2::-1]))      # the order matters in fp32
    # an equivariant "prediction": every variant carried back is the tile itself, the mean of K copies
    e = I.d4_elements("d4")
    back = [R.carried_back(R.window_transform(tiles[0], x), x) for x in e]
    assert all(np.array_equal(b, tiles[0]) for b in back)


def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", hdr)
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    proto = re.search(r"\bint\s+" + ENTRY + r"\s*\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[ENTRY][1]) == 18          # one binding argument per parameter
    lib.jspsr_abi_version.restype = ctypes.c_int
    assert lib.jspsr_abi_version() == 25 == _lib.load().jspsr_abi_version()
    assert "K16 (ABI v25, additive)" in hdr
    assert all(callable(getattr(I, name)) for name in ("launch_prepare_windows_d4", "prepare_windows_d4", "mean_windows"))


def test_entry_refuses_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN with a message that names the entry, before a launch (safe without a GPU: no pointer is
    dereferenced on the device, the host arrays are real)."""
    lib = _lib.load()
    x = ctypes.c_void_p(4096)
    n0 = lib.jspsr_launch_count(b"scene_prepare_windows_d4")

    def message():
        return lib.jspsr_last_error().decode()

    six_p, six_ll, six_i = ctypes.c_void_p * 6, ctypes.c_longlong * 6, ctypes.c_int * 6
    src, nbytes, out = six_p(), six_ll(), six_p()
    ch, coff, pitch = six_i(), six_i(), six_i()
    two = ctypes.c_int * 2

    def prepare(B=2, kh=24, kw=16, samples=x, scenes=x, codes=two(0, 2), mask_div=3, flags=0, src=src):
        return lib.jspsr_scene_prepare_windows_d4(src, nbytes, out, ch, coff, pitch, scenes, 1, samples, codes, B, kh, kw, flags,
                                                  -80.0, 933.0, mask_div, None)

    def refused(code, *words, **kw):
        assert prepare(**kw) == code, kw
        assert "scene_prepare_windows_d4" in message() and all(w in message() for w in words), (kw, message())

    out[5], ch[5], pitch[5] = 4096, 2, 2                                        # coord alone: no store needed
    for kw in (dict(B=0), dict(B=-1), dict(kh=0), dict(kw=0), dict(kw=-4), dict(samples=None), dict(scenes=None), dict(codes=None),
               dict(src=None), dict(mask_div=0), dict(flags=64)):
        refused(-1, **kw)
    refused(-1, "65535", B=65536, codes=(ctypes.c_int * 65536)())
    refused(-1, "image range", flags=4 | 16)
    refused(-1, "outside 0..15", codes=two(0, 16))
    refused(-1, "outside 0..15", codes=two(-1, 0))
    refused(-1, "one parity", codes=two(0, 4))
    refused(-1, "one parity", codes=two(14, 10))
    refused(-2, "aligned", samples=ctypes.c_void_p(4098))
    refused(-2, "aligned", scenes=ctypes.c_void_p(4100))
    ch[5] = 3
    refused(-1, "bad channels")                                                 # coord has two channels
    ch[5], pitch[5] = 2, 1
    refused(-1, "bad channels")                                                 # the pitch does not hold them
    ch[5], pitch[5], coff[5] = 2, 2, -1
    refused(-1, "bad channels")
    coff[5] = 0
    out[5] = 4098
    refused(-2, "aligned")
    out[5] = None
    refused(-1, "no output")
    out[1], ch[1], pitch[1] = 4096, 1, 1
    refused(-1, "hr_dem")
    out[1] = None
    out[3], ch[3], pitch[3] = 4096, 2, 2
    refused(-1, "store")                                                        # a mask output and no mask store
    ch[3], pitch[3] = 17, 17
    refused(-1, "bad channels")
    src[3], nbytes[3], ch[3], pitch[3] = 4098, 64, 2, 2
    refused(-2, "store not 4-byte aligned")
    assert lib.jspsr_launch_count(b"scene_prepare_windows_d4") == n0


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
    with pytest.raises(ValueError, match="window_tta.*tile"):
        I.predict_scenes(model, big, window_tta="d4")
    with pytest.raises(ValueError, match="window_tta together with tta"):
        I.predict_scenes(model, big, tile=32, tta="d4", window_tta="d4")
    with pytest.raises(ValueError, match="window_tta together with tta"):
        I.predict_scenes(model, big, tile=32, tta=[0], window_tta=[(1, False, False)])
    with pytest.raises(ValueError, match="rot90 must be 0..3"):
        I.predict_scenes(model, big, tile=32, window_tta=[(4, False, False)])
    with pytest.raises(ValueError, match="outside 0..15"):
        I.predict_scenes(model, big, tile=32, window_tta=[16])
    with pytest.raises(ValueError, match="same element"):
        I.predict_scenes(model, big, tile=32, window_tta=[0, 11])
    with pytest.raises(ValueError, match="'d4'"):
        I.predict_scenes(model, big, tile=32, window_tta="d8")
    with pytest.raises(ValueError, match="no elements"):
        I.predict_scenes(model, big, tile=32, window_tta=[])
    with pytest.raises(NotImplementedError, match="tile together with tta"):    # as before
        I.predict_scenes(model, big, tile=32, tta="d4")
    with pytest.raises(ValueError, match="multiple of the model's 8"):          # the tile's own checks still come
        I.predict_scenes(model, big, tile=36, window_tta="d4")
    with pytest.raises(ValueError, match="pad must be 0"):
        I.predict_scenes(model, big, tile=32, pad=4, window_tta="d4")
