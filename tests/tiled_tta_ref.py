"""TEST INFRASTRUCTURE ONLY -- numpy restatement of K16 (csrc/scene_prepare.hip, jspsr_amd/infer.py: prepare_windows_d4,
mean_windows): the transform of a window, the index map behind it, and the mean of a window's predictions."""
import numpy as np

from jspsr_amd import infer as I


def d4_source(code, H, W, i, j):
    """Pixel (i, j) of flipud?(fliplr?(rot90(m, rot90))) is pixel (sy, sx) of the H x W raster m; code = rot90 * 4 +
    flip_lr * 2 + flip_ud.  The kernels' map (csrc/d4.h), restated."""
    rot, lr, ud = code >> 2, bool(code & 2), bool(code & 1)
    oh, ow = (W, H) if rot % 2 else (H, W)
    i2 = oh - 1 - i if ud else i
    j2 = ow - 1 - j if lr else j
    if rot == 0:
        return i2, j2
    if rot == 1:
        return j2, W - 1 - i2
    if rot == 2:
        return H - 1 - i2, W - 1 - j2
    return H - 1 - j2, i2


def window_transform(cut, element, axes=(-2, -1)):
    """The transformed window: `infer.d4_apply` on the cut (..., kh, kw)."""
    axes = tuple(a % cut.ndim for a in axes)
    return np.ascontiguousarray(I.d4_apply(cut, element, axes=axes))


def carried_back(pred, element, axes=(-2, -1)):
    """A prediction (..., oh, ow) of a transformed window, upright again."""
    axes = tuple(a % pred.ndim for a in axes)
    return np.ascontiguousarray(I.d4_invert(pred, element, axes=axes), dtype=np.float32)


def mean_tiles(upright):
    """upright[k] (N, kh, kw) fp32, the predictions carried back, in element order -> (((y_0 + y_1) + y_2) + ...) / fp32(K):
    fp32 additions one after the other, one fp32 division."""
    acc = None
    for y in upright:
        y = np.asarray(y, dtype=np.float32)
        acc = y.copy() if acc is None else (acc + y).astype(np.float32)
    return (acc / np.float32(len(upright))).astype(np.float32)
