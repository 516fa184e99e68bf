"""numpy restatements for the void tests (K17): the nearest-seed rule by brute force, the two-phase scheme that the kernels
run, the fill, the margin mask and the by-hand route that `InferenceScenes(nodata=...)` + `predict_scenes` replace.  numpy
only.

The rule: for a query pixel (y, x) the seed of the same scene that minimises (dy^2 + dx^2, |dx|, dx, dy) lexicographically,
d = seed - query -> src = y_s * W + x_s and d2; -1 / -1 without a seed, or with none within `limit` (d2 > limit^2)."""
import numpy as np


def void_pixels(a, nodata):
    """Not finite, or (unless nodata is NaN) equal to np.float32(nodata)."""
    a = np.asarray(a, dtype=np.float32)
    v = ~np.isfinite(a)
    nd = np.float32(nodata)
    return v if np.isnan(nd) else v | (a == nd)


def nearest_seed_ref(seed, limit=None):
    """Brute force, every seed against every query, the lexicographic minimum taken key by key -> (src, d2) int32 (H, W)."""
    seed = np.asarray(seed) != 0
    H, W = seed.shape
    ys, xs = (c.astype(np.int64) for c in np.nonzero(seed))
    src = np.full((H, W), -1, dtype=np.int32)
    d2 = np.full((H, W), -1, dtype=np.int32)
    if len(ys) == 0:
        return src, d2
    for y in range(H):
        for x in range(W):
            dy, dx = ys - y, xs - x
            d = dy * dy + dx * dx
            c = np.flatnonzero(d == d.min())
            for key in (np.abs(dx), dx, dy):
                c = c[key[c] == key[c].min()]
            assert len(c) == 1
            j = c[0]
            if limit is not None and d[j] > limit * limit:
                continue
            src[y, x], d2[y, x] = ys[j] * W + xs[j], d[j]
    return src, d2


_MEMO = {}


def nearest_seed_memo(seed, limit=None):
    """`nearest_seed_ref`, computed once per (mask, limit); the arrays are shared, nobody writes to them."""
    seed = np.ascontiguousarray(np.asarray(seed) != 0)
    key = (seed.shape, seed.tobytes(), limit)
    if key not in _MEMO:
        _MEMO[key] = nearest_seed_ref(seed, limit)
    return _MEMO[key]


def d2_min_ref(seed):
    """The minimum over ALL seeds of the squared distance alone, no search order and no early exit: the minimum over the
    seeds of a column first (every row against every row), then over the columns (every column against every column) --
    min over (y', x') = min over x' of min over y'.  (H, W) int64, -1 without a seed."""
    seed = np.asarray(seed) != 0
    H, W = seed.shape
    if not seed.any():
        return np.full((H, W), -1, dtype=np.int64)
    big = np.int64(4) * (H + W) ** 2                                              # above every real distance
    r = np.arange(H, dtype=np.int64)
    dy2 = (r[:, None] - r[None, :]) ** 2                                          # [query row][seed row]
    col = np.where(seed.T[None, :, :], dy2[:, None, :], big).min(axis=2)          # [y][x']: the column's nearest seed
    c = np.arange(W, dtype=np.int64)
    dx2 = (c[:, None] - c[None, :]) ** 2                                          # [x][x']
    return (col[:, None, :] + dx2[None, :, :]).min(axis=2)


def column_distance(seed):
    """Phase 1: per pixel (row of the column's nearest seed) - (own row), ties to the upper seed; None-marker: H + W + 1."""
    seed = np.asarray(seed) != 0
    H, W = seed.shape
    none = H + W + 1
    g = np.full((H, W), none, dtype=np.int64)
    for x in range(W):
        rows = np.flatnonzero(seed[:, x])
        for y in range(H):
            if len(rows):
                dist = np.abs(rows - y)
                g[y, x] = rows[np.flatnonzero(dist == dist.min())[0]] - y          # the first of two is the upper one
    return g, none


def two_phase(seed, limit=None):
    """The scheme the kernels run, restated pixel by pixel: phase 1 per column, phase 2 the walk x, x-1, x+1, x-2, ... over
    k^2 + g^2 with strict improvements, until k^2 >= best or k > limit -> (src, d2) int32 (H, W)."""
    seed = np.asarray(seed) != 0
    H, W = seed.shape
    g, none = column_distance(seed)
    src = np.full((H, W), -1, dtype=np.int32)
    d2 = np.full((H, W), -1, dtype=np.int32)
    for y in range(H):
        for x in range(W):
            best, bx = None, -1
            if g[y, x] != none:
                best, bx = int(g[y, x]) ** 2, x
            k = 1
            while (best is None or k * k < best) and (limit is None or k <= limit) and (x - k >= 0 or x + k < W):
                for xx in (x - k, x + k):
                    if 0 <= xx < W and g[y, xx] != none:
                        d = k * k + int(g[y, xx]) ** 2
                        if best is None or d < best:
                            best, bx = d, xx
                k += 1
            if best is not None and (limit is None or best <= limit * limit):
                src[y, x], d2[y, x] = (y + g[y, bx]) * W + bx, best
    return src, d2


def fill_ref(dem, void, base, limit=None):
    """dem (H, W) fp32 with its voids replaced: the nearest valid pixel's value; np.float32(base) where none is within
    `limit` (0: everywhere)."""
    dem = np.asarray(dem, dtype=np.float32)
    void = np.asarray(void, dtype=bool)
    out = dem.copy()
    if limit == 0:
        out[void] = np.float32(base)
        return out
    src, _ = nearest_seed_memo(~void, limit)
    take = dem.reshape(-1)[np.maximum(src, 0)]
    out[void] = np.where(src >= 0, take, np.float32(base))[void]
    return out


def margin_ref(void, margin):
    """void, or within the Euclidean distance `margin` of a void."""
    void = np.asarray(void, dtype=bool)
    if margin == 0:
        return void.copy()
    return nearest_seed_memo(void, margin)[1] >= 0


def by_hand_store(lr_dems, nodata, relative, void_margin=0, fill_limit=None):
    """What a user does on the host without the feature: per (H, W, 1) scene detect the voids, take the base over the valid
    pixels, fill -> (filled (H, W, 1) scenes, bases, voids (H, W), output masks (H, W))."""
    filled, bases, voids, outs = [], [], [], []
    for a in lr_dems:
        a = np.asarray(a, dtype=np.float32)
        v = void_pixels(a[..., 0], nodata)
        base = np.min(a[..., 0][~v]) if relative else 0
        filled.append(fill_ref(a[..., 0], v, base, fill_limit)[..., None])
        bases.append(base)
        voids.append(v)
        outs.append(margin_ref(v, void_margin))
    return filled, bases, voids, outs
