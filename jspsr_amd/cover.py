"""The cover of a scene of any size by equal tiles, and the ramp weights that merge the tiles' predictions (host, numpy).

The reference cuts a square sample into 2 x 2 or 3 x 3 tiles and stitches the predictions with linear ramps over the
overlaps (`TileCrop`, data/data_utils.py:87-194; `gen_weight_row/col` + `merge_dem`, utils/utils.py:802-967; here
`tiles.py`).  `plan_cover` continues that rule to any H x W scene and any tile, per axis of length L with tile side k:

  origins   L == k: one tile at 0.  Otherwise n = ceil((L - overlap) / (k - overlap)) tiles at o_i = (i * (L - k)) // (n - 1):
            the first starts at 0, the last ends at L, and neighbours share at least `overlap` pixels.
  extent    tile i is used on [a_i, b_i): a_0 = 0, else a_i = o_i + trim; b_{n-1} = L, else b_i = o_i + k - trim.  `trim`
            pixels are dropped on the sides that face another tile (where the zero padding of the tile's convolutions
            shows), never on the scene's edge.
  seams     seam i, between tiles i and i + 1, is [s_i, e_i) with e_i = b_i and s_i = max(a_{i+1}, e_{i-1}), e_{-1} = 0:
            tile i + 1 has weight 0 before s_i, so at most two tiles meet anywhere.  In a seam of width p tile i gets
            linspace(1, 0, p + 2, float64)[1:-1] cast to fp32 -- `tiles._weight_1d`'s table -- and tile i + 1 the reversed
            ramp; elsewhere inside its extent a tile's weight is 1, outside 0.

The two-dimensional weight of tile (ty, tx) at its pixel (j, i) is wx[tx][i] * wy[ty][j], applied as (m * wx) * wy.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Cover = namedtuple("Cover", "H W kh kw overlap trim oy ox wy wx lo_y lo_x")
Cover.__doc__ = """plan_cover's result.  oy (n_y,), ox (n_x,) int32 tile origins; wy (n_y, kh), wx (n_x, kw) fp32 weights of
every tile row / column; lo_y (H,), lo_x (W,) int32, the lowest tile index with a non-zero weight at that coordinate.
`windows()` lists the tiles' corners row-major."""
Cover.n_y = property(lambda self: len(self.oy))
Cover.n_x = property(lambda self: len(self.ox))
Cover.n = property(lambda self: len(self.oy) * len(self.ox))
Cover.windows = lambda self: [(int(y), int(x)) for y in self.oy for x in self.ox]
Cover.key = property(lambda self: (self.H, self.W, self.kh, self.kw, self.overlap, self.trim))


def ramp(p: int) -> np.ndarray:
    """The falling ramp of a seam of width p: linspace(1, 0, p + 2) in float64 without its ends, as fp32."""
    return np.linspace(1, 0, p + 2, dtype=np.float64)[1:-1].astype(np.float32)


def axis_cover(L: int, k: int, overlap: int, trim: int = 0):
    """One axis -> (origins (n,) int32, weights (n, k) fp32, lo (L,) int32)."""
    L, k, overlap, trim = int(L), int(k), int(overlap), int(trim)
    if L < 1 or k < 1 or overlap < 0 or trim < 0:
        raise ValueError(f"plan_cover: side {L}, tile {k}, overlap {overlap}, trim {trim}")
    if L < k:
        raise ValueError(f"plan_cover: a side of {L} is below the tile side {k}; pass a rectangular tile=(kh, kw) that fits")
    if overlap < 2 * trim:
        raise ValueError(f"plan_cover: overlap {overlap} is below twice the trim {trim}")
    if overlap >= k:
        raise ValueError(f"plan_cover: overlap {overlap} is not below the tile side {k}")
    if L == k:
        return np.zeros(1, np.int32), np.ones((1, k), np.float32), np.zeros(L, np.int32)
    n = -(-(L - overlap) // (k - overlap))
    o = [(i * (L - k)) // (n - 1) for i in range(n)]
    a = [0 if i == 0 else o[i] + trim for i in range(n)]
    b = [L if i == n - 1 else o[i] + k - trim for i in range(n)]
    w = np.zeros((n, k), np.float32)
    for i in range(n):
        w[i, a[i] - o[i]:b[i] - o[i]] = 1.0
    e_prev = 0
    for i in range(n - 1):
        s, e = max(a[i + 1], e_prev), b[i]
        r = ramp(e - s)
        w[i, s - o[i]:e - o[i]] = r
        w[i + 1, :s - o[i + 1]] = 0.0
        w[i + 1, s - o[i + 1]:e - o[i + 1]] = r[::-1]
        e_prev = e
    lo = np.full(L, -1, np.int32)
    for i in reversed(range(n)):
        lo[o[i] + np.flatnonzero(w[i])] = i
    assert (lo >= 0).all()
    return np.asarray(o, np.int32), w, lo


def plan_cover(H: int, W: int, tile, overlap: int, trim: int = 0) -> Cover:
    """The cover of an H x W scene by tiles of `tile` (an int, or (kh, kw)) -> `Cover`.  ValueError: overlap < 2 * trim,
    overlap >= a tile side, a scene side below its tile side."""
    kh, kw = (int(tile), int(tile)) if isinstance(tile, (int, np.integer)) else (int(tile[0]), int(tile[1]))
    oy, wy, lo_y = axis_cover(H, kh, overlap, trim)
    ox, wx, lo_x = axis_cover(W, kw, overlap, trim)
    return Cover(int(H), int(W), kh, kw, int(overlap), int(trim), oy, ox, wy, wx, lo_y, lo_x)
