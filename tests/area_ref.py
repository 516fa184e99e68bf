"""K26 restated in numpy int64: the exact area downsample of HWC uint8 rasters (csrc/area.hip, resample.area_rasters).

One axis, output length H over a source of h, 1 <= H <= h: in units where a source pixel has length H, output Y covers
[Y h, (Y + 1) h) and source pixel i covers [i H, (i + 1) H); the weight is the overlap where positive.  With S = A_y v A_x^T
per channel and D = h w, "area" is (S + D // 2) // D and "majority" the rule of `majority` below.  D * 255 stays below 2^41:
int64 holds every sum."""
import numpy as np


def overlap(h: int, H: int, Y, i) -> np.ndarray:
    """a(Y, i) = min((Y + 1) h, (i + 1) H) - max(Y h, i H) where positive, else 0, for index arrays that broadcast; an i
    outside 0 .. h - 1 is no pixel and gives 0."""
    assert 1 <= H <= h
    Y, i = np.asarray(Y, dtype=np.int64), np.asarray(i, dtype=np.int64)
    a = np.maximum(np.minimum((Y + 1) * h, (i + 1) * H) - np.maximum(Y * h, i * H), 0)
    return np.where((i >= 0) & (i < h), a, 0)


def axis_matrix(h: int, H: int) -> np.ndarray:
    """The dense (H, h) int64 weight matrix, straight from the overlap formula."""
    return overlap(h, H, np.arange(H)[:, None], np.arange(h)[None, :])


def coverage(img_hwc: np.ndarray, H: int, W: int) -> np.ndarray:
    """S = sum_y sum_x a_y a_x v per channel, (H, W, C) int64."""
    h, w, _ = img_hwc.shape
    ay, ax = axis_matrix(h, H), axis_matrix(w, W)
    v = img_hwc.astype(np.int64)
    rows = np.einsum("yi,ijc->yjc", ay, v)                        # (H, w, C)
    return np.einsum("xj,yjc->yxc", ax, rows)


def area_u8(img_hwc: np.ndarray, H: int, W: int) -> np.ndarray:
    """(A_y img A_x^T + D // 2) // D per channel -> (H, W, C) uint8: the area mean, rounded half up."""
    h, w, _ = img_hwc.shape
    D = h * w
    out = (coverage(img_hwc, H, W) + D // 2) // D
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def majority(mask_hwc: np.ndarray, H: int, W: int) -> np.ndarray:
    """The one-hot mask on the coarse grid: a non-zero byte counts as 1; none = D - sum_c S_c (signed); the pixel is one-hot
    at c*, the lowest index among the channels of largest S_c, iff S_c* > 0 and S_c* >= none; otherwise all zeros."""
    h, w, C = mask_hwc.shape
    D = h * w
    S = coverage((mask_hwc != 0).astype(np.uint8), H, W)
    none = D - S.sum(axis=2)
    best = S[..., 0].copy()
    star = np.zeros((H, W), dtype=np.int64)
    for c in range(1, C):                                         # strictly larger only: the lowest index wins a tie
        better = S[..., c] > best
        best = np.where(better, S[..., c], best)
        star = np.where(better, c, star)
    hot = (best > 0) & (best >= none)
    out = np.zeros((H, W, C), dtype=np.uint8)
    for c in range(C):
        out[..., c] = (hot & (star == c)).astype(np.uint8)
    return out
