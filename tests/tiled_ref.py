"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the K15 cover (jspsr_amd/cover.py) and merge (csrc/scene_tiles.hip),
written independently of the package: the planner's rule per axis from its statement (origins, effective extents, seams,
ramps), and the merge as a loop over the tiles, row-major, in float32 with one rounding per operation -- acc starts at 0
and takes acc + (m * wx) * wy for every tile whose weights at the pixel are not zero.  CPU only.
"""
from __future__ import annotations

import math

import numpy as np


def axis(L, k, overlap, trim=0):
    """-> (origins list, weights (n, k) fp32, lo (L,) int32) of one axis."""
    if L == k:
        return [0], np.ones((1, k), np.float32), np.zeros(L, np.int32)
    n = math.ceil((L - overlap) / (k - overlap))
    o = [(i * (L - k)) // (n - 1) for i in range(n)]
    a = [0] + [o[i] + trim for i in range(1, n)]
    b = [o[i] + k - trim for i in range(n - 1)] + [L]
    full = np.zeros((n, L), np.float32)                              # the weights over the whole axis, then cut to the tiles
    for i in range(n):
        full[i, a[i]:b[i]] = 1
    e_prev = 0
    for i in range(n - 1):
        s, e = max(a[i + 1], e_prev), b[i]
        r = np.linspace(1, 0, e - s + 2, dtype=np.float64)[1:-1].astype(np.float32)
        full[i, s:e] = r
        full[i + 1, :s] = 0
        full[i + 1, s:e] = r[::-1]
        e_prev = e
    w = np.stack([full[i, o[i]:o[i] + k] for i in range(n)])
    assert all(not full[i, :o[i]].any() and not full[i, o[i] + k:].any() for i in range(n))      # nothing outside the tile
    lo = np.array([int(np.flatnonzero(full[:, x])[0]) for x in range(L)], np.int32)
    return o, w, lo


def cover(H, W, tile, overlap, trim=0):
    kh, kw = (tile, tile) if isinstance(tile, int) else tile
    oy, wy, lo_y = axis(H, kh, overlap, trim)
    ox, wx, lo_x = axis(W, kw, overlap, trim)
    return dict(H=H, W=W, kh=kh, kw=kw, oy=oy, ox=ox, wy=wy, wx=wx, lo_y=lo_y, lo_x=lo_x)


def merge(m: np.ndarray, c: dict) -> np.ndarray:
    """m (n_y * n_x, kh, kw) float32, the tiles of one scene row-major (in metres, or whatever is to be feathered) ->
    (H, W) float32.  A tile is not read where its weight is zero (np.where drops it, NaN or not)."""
    assert m.dtype == np.float32 and m.shape == (len(c["oy"]) * len(c["ox"]), c["kh"], c["kw"])
    out = np.zeros((c["H"], c["W"]), np.float32)
    for ty, y0 in enumerate(c["oy"]):
        for tx, x0 in enumerate(c["ox"]):
            wy, wx = c["wy"][ty][:, None], c["wx"][tx][None, :]
            t = m[ty * len(c["ox"]) + tx]
            live = (wy != 0) & (wx != 0)
            with np.errstate(invalid="ignore"):
                term = ((t * wx).astype(np.float32) * wy).astype(np.float32)
            view = out[y0:y0 + c["kh"], x0:x0 + c["kw"]]
            view[...] = np.where(live, (view + term).astype(np.float32), view)
    return out
