"""The self-ensemble (K14) without a GPU: the D4 elements and their inverse in `jspsr_amd.infer`, the frame of a transposed
scene, and the two entry points in the header, the built library and the binding.  Everything is compared with ==."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from jspsr_amd import _lib
from jspsr_amd import infer as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("jspsr_scene_prepare_d4", "jspsr_scene_finish_mean")


def numpy_d4(a, r, lr, ud):
    """RandomFlipRotate90's order (data/data_utils.py:26-28)."""
    a = np.rot90(a, r)
    a = np.fliplr(a) if lr else a
    return np.flipud(a) if ud else a


def test_d4_is_eight_distinct_elements():
    els = I.d4_elements("d4")
    assert els == [(r, lr, False) for r in range(4) for lr in (False, True)]
    a = np.array([[1, 2], [3, 4], [5, 6]])                                      # asymmetric: no element but the identity fixes it
    images = [I.d4_apply(a, e) for e in els]
    for e, t in zip(els, images):
        assert np.array_equal(t, numpy_d4(a, *e)), e
        assert t.shape == ((2, 3) if e[0] % 2 else (3, 2))
    assert len({(t.shape, t.tobytes()) for t in images}) == 8
    assert I.d4_elements(None) == [(0, False, False)]
    assert I.d4_elements([(3, True, False), 7]) == [(3, True, False), (1, True, True)]     # the order given; codes become triples
    assert [I.d4_code(e) for e in els] == [0, 2, 4, 6, 8, 10, 12, 14]


def test_sixteen_codes_are_eight_classes_and_duplicates_are_refused():
    a = np.arange(6).reshape(3, 2)
    classes = {}
    for code in range(16):
        r, lr, ud = code >> 2, bool(code & 2), bool(code & 1)
        t = I.d4_apply(a, code)
        assert np.array_equal(t, numpy_d4(a, r, lr, ud)), code
        classes.setdefault((t.shape, t.tobytes()), []).append(code)
        assert np.array_equal(I.d4_apply(a, I.d4_canonical(code)), t) and I.d4_canonical(code)[2] is False
    assert len(classes) == 8 and all(len(v) == 2 for v in classes.values())
    for pair in classes.values():                                               # the two codes of a class, as codes and triples
        with pytest.raises(ValueError, match="same element"):
            I.d4_elements(pair)
        with pytest.raises(ValueError, match="same element"):
            I.d4_elements([(c >> 2, bool(c & 2), bool(c & 1)) for c in pair])
    with pytest.raises(ValueError, match="same element"):
        I.d4_elements(list(range(0, 16, 2)) + [1])
    for bad in ([16], [-1], [(4, False, False)], [(0, 2, False)], [(0, False)], "d8", [], [None], [(1.5, False, False)]):
        with pytest.raises(ValueError):
            I.d4_elements(bad)


def test_inverse_undoes_every_element():
    a = np.arange(15).reshape(5, 3)
    stack = np.arange(2 * 15 * 4).reshape(2, 5, 3, 4)
    for code in range(16):
        assert np.array_equal(I.d4_invert(I.d4_apply(a, code), code), a), code
        assert np.array_equal(I.d4_apply(I.d4_invert(a, code), code), a), code
        t = I.d4_apply(stack, code, axes=(1, 2))
        assert t.shape == ((2, 3, 5, 4) if code & 4 else (2, 5, 3, 4))
        assert np.array_equal(t[1, ..., 2], I.d4_apply(stack[1, ..., 2], code))
        assert np.array_equal(I.d4_invert(t, code, axes=(1, 2)), stack), code


def test_transposed_frame_is_the_frame_of_the_transposed_shape():
    rows, cols, top, left = I.frame_maps(13, 10, 3, 8)
    assert (len(rows), len(cols), top, left) == (24, 16, 3, 3)
    trows, tcols, ttop, tleft = I.frame_maps(10, 13, 3, 8)
    assert (len(trows), len(tcols), ttop, tleft) == (16, 24, 3, 3)
    # padding comes after the transform: the transposed frame is NOT the transpose of the frame (the bottom strip sits one
    # row above a mirror, the right strip does not)
    a = np.arange(130).reshape(13, 10)
    frame = a[rows.astype(np.int64)][:, cols.astype(np.int64)]
    tframe = I.d4_apply(a, (1, False, False))[trows.astype(np.int64)][:, tcols.astype(np.int64)]
    assert tframe.shape == (16, 24) and not np.array_equal(tframe, I.d4_apply(frame, (1, False, False)))
    assert np.array_equal(tframe[3:13, 3:16], np.rot90(a))
    # a scene whose transposed shape cannot fill the border: frame_maps' ValueError, the element named
    assert len(I.frame_maps(12, 4, 4, 1)[0]) == 20
    with pytest.raises(ValueError, match=r"frame_maps: element \(1, False, False\)"):
        I._frame_d4(types.SimpleNamespace(device="cpu"), 12, 4, 1, 4, 1, (1, False, False))


def test_header_library_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "replaces" in hdr[hdr.index("jspsr_scene_prepare_d4:"):hdr.index("#define JSPSR_TTA_MAX_VARIANTS")]
    assert re.search(r"#define\s+JSPSR_TTA_MAX_VARIANTS\s+8\b", hdr)
    lib.jspsr_abi_version.restype = ctypes.c_int
    assert lib.jspsr_abi_version() == _lib.ABI_VERSION == _lib.load().jspsr_abi_version()
    assert ctypes.sizeof(_lib.TtaVariant) == 40                                 # a pointer and eight ints, as the header lays them out
    fields = re.search(r"typedef struct jspsr_tta_variant \{(.*?)\}", hdr, re.S).group(1)
    assert [f for f, _ in _lib.TtaVariant._fields_] == re.findall(r"\b(pred|dtype|code|Hp|Wp|top|left|h|w)\b", fields)


def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN with a message, before a launch (safe without a GPU; no pointer is dereferenced on the
    device, the host arrays are real)."""
    lib = _lib.load()
    x = ctypes.c_void_p(4096)
    V = _lib.TtaVariant

    def finish(variants, K=None, B=1, H=13, W=10, out=x):
        arr = (V * max(len(variants), 1))(*variants)
        return lib.jspsr_scene_finish_mean(arr, len(variants) if K is None else K, out, x, B, H, W, 1, 1, -80.0, 933.0, None)

    def message():
        return lib.jspsr_last_error().decode()

    even, odd = V(4096, 0, 0, 24, 16, 3, 3, 13, 10), V(4096, 0, 4, 16, 24, 3, 3, 10, 13)
    assert finish([]) == -1 and "scene_finish_mean" in message()
    assert finish([even] * 9) == -1 and "9 variants" in message()
    assert lib.jspsr_scene_finish_mean(None, 1, x, x, 1, 13, 10, 1, 1, -80.0, 933.0, None) == -1
    assert finish([even], B=0) == -1 and finish([even], H=0) == -1 and finish([even], out=None) == -1
    assert finish([even, V(4096, 0, 11, 24, 16, 3, 3, 13, 10)]) == -1 and "same element" in message()      # 0 and (2, lr, ud)
    assert finish([even, odd, even]) == -1 and "same element" in message()
    assert finish([V(4096, 0, 0, 24, 16, 12, 3, 13, 10)]) == -1 and "leaves" in message()
    assert finish([V(4096, 0, 0, 24, 16, 3, -1, 13, 10)]) == -1 and "leaves" in message()
    assert finish([V(4096, 0, 4, 24, 16, 3, 3, 13, 10)]) == -1 and "transforms to 10 x 13" in message()    # the untransposed frame
    assert finish([V(4096, 0, 0, 16, 24, 3, 3, 10, 13)]) == -1 and "transforms to 13 x 10" in message()
    assert finish([V(4096, 2, 0, 24, 16, 3, 3, 13, 10)]) == -1                                             # neither fp32 nor bf16
    assert finish([V(4096, 0, 16, 24, 16, 3, 3, 13, 10)]) == -1 and finish([V(None, 0, 0, 24, 16, 3, 3, 13, 10)]) == -1
    assert finish([V(4098, 0, 0, 24, 16, 3, 3, 13, 10)]) == -2 and "aligned" in message()
    assert finish([V(4097, 1, 0, 24, 16, 3, 3, 13, 10)]) == -2
    assert finish([even], out=ctypes.c_void_p(4098)) == -2

    six_p, six_ll, six_i = ctypes.c_void_p * 6, ctypes.c_longlong * 6, ctypes.c_int * 6
    src, nbytes, out = six_p(), six_ll(), six_p()
    ch, coff, pitch = six_i(), six_i(), six_i()

    def prepare(codes=(0, 2), B=None, Hp=24, Wp=16, rows=x, mask_div=3, flags=0, host=True):
        arr = (ctypes.c_int * max(len(codes), 1))(*codes)
        return lib.jspsr_scene_prepare_d4(src, nbytes, out, ch, coff, pitch, x, 1, x, arr if host else None,
                                          len(codes) if B is None else B, rows, x, Hp, Wp, flags, -80.0, 933.0, mask_div, None)

    out[5], ch[5], pitch[5] = 4096, 2, 2                                        # coord alone: no store needed
    assert prepare(B=0) == -1 and "scene_prepare_d4" in message()
    assert prepare(host=False) == -1 and prepare(Hp=0) == -1 and prepare(rows=None) == -1 and prepare(mask_div=0) == -1
    assert prepare(flags=64) == -1 and prepare(codes=[0] * 2, B=65536) == -1
    assert prepare(codes=(0, 16)) == -1 and "outside 0..15" in message()
    assert prepare(codes=(0, -1)) == -1
    for mixed in ((0, 4), (8, 2, 13), (6, 6, 10)):
        assert prepare(codes=mixed) == -1 and "one parity" in message(), mixed
    out[5] = None
    assert prepare() == -1 and "no output" in message()
    out[1], ch[1], pitch[1] = 4096, 1, 1
    assert prepare() == -1 and "hr_dem" in message()
    out[1] = None
    out[3], ch[3], pitch[3] = 4096, 2, 2
    assert prepare() == -1 and "store" in message()
    out[3], ch[3], pitch[3] = 4098, 2, 2
    assert prepare() == -2
