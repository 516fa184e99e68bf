"""The independent restatement of the error distribution (K21), built from the RAW errors and never from a histogram: what
the reference's summarise_evaluation does for its figure (utils/utils.py:1394-1456) -- the numpy filter lo <= e <= hi,
`astype("float16")` -- then np.unique over the uint16 view for the counts, and the curve of seaborn's kdeplot as a direct
fp64 sum over all n points: scipy's gaussian_kde bandwidth (Scott's factor n^(-1/5) times the ddof-1 standard deviation,
times bw_adjust) on seaborn's support grid (min - cut bw .. max + cut bw, np.linspace)."""
import numpy as np


def f16_key(bits):
    bits = np.asarray(bits).astype(np.int64)
    return np.where(bits & 0x8000, bits ^ 0xffff, bits ^ 0x8000)


def exhaustive_values():
    """float32 operands that exercise every float16 rounding decision: every finite float16 value, the fp32 point halfway to
    its upper neighbour, that point's two fp32 neighbours; +-0, the subnormal range's edges, +-5, nextafter(5, inf), 4.999
    (rounds to 5.0), and values far outside."""
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    h = bits.view(np.float16)
    h = h[np.isfinite(h)]
    v = h.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        up = np.nextafter(h, np.float16(np.inf)).astype(np.float32)
        mid = ((v.astype(np.float64) + up.astype(np.float64)) * 0.5).astype(np.float32)       # exact: 12 bits of mantissa at most
    mid = mid[np.isfinite(mid)]
    extra = np.array([0.0, -0.0, 5.0, -5.0, np.nextafter(np.float32(5), np.float32(np.inf)), np.nextafter(np.float32(-5), np.float32(-np.inf)),
                      4.999, -4.999, 2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -26, -2.0 ** -25,
                      2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0)), 1e-30, -1e-30, 1e-45, 65504.0, 65519.99, 1e30, -1e30],
                     dtype=np.float32)
    return np.concatenate([v, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)), extra]).astype(np.float32)


def bins(lo, hi):
    k = f16_key(np.array([lo, hi], dtype=np.float32).astype(np.float16).view(np.uint16))
    return int(k[0]), int(k[1] - k[0] + 1)


def histogram(e, lo=-5.0, hi=5.0):
    """float32 errors (already compacted by any mask) -> (hist (K,) int64, (n_scored, n_in, n_below, n_above), key0)."""
    e = np.asarray(e, dtype=np.float32).reshape(-1)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    key0, K = bins(lo, hi)
    with np.errstate(invalid="ignore"):
        inside = (e >= lo32) & (e <= hi32)
        below, above = int((e < lo32).sum()), int((e > hi32).sum())
    u, n = np.unique(e[inside].astype("float16").view(np.uint16), return_counts=True)
    hist = np.zeros(K, dtype=np.int64)
    np.add.at(hist, np.clip(f16_key(u) - key0, 0, K - 1), n)                    # lo = +0 keeps -0: the same value
    return hist, (e.size, int(inside.sum()), below, above), key0


def clipped(e, lo=-5.0, hi=5.0):
    """The reference's column: the errors inside [lo, hi] as float16, promoted to float64 (what seaborn hands to scipy)."""
    e = np.asarray(e, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return e[(e >= np.float32(lo)) & (e <= np.float32(hi))].astype("float16").astype(np.float64)


def curve(x, gridsize=200, cut=0.5, bw_adjust=1.0, block=2048):
    """x: float64 points -> (support, density, (mean, std, bw)); a direct sum over all n points."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    nan = np.full(gridsize, np.nan)
    if n < 2 or np.var(x, ddof=1) == 0:
        return nan, nan, (x.mean() if n else np.nan, np.std(x, ddof=1) if n > 1 else np.nan, np.nan)
    sd = np.std(x, ddof=1)
    bw = sd * n ** (-1.0 / 5.0) * bw_adjust
    support = np.linspace(x.min() - cut * bw, x.max() + cut * bw, gridsize)
    dens = np.zeros(gridsize)
    for i in range(0, n, block):
        d = support[:, None] - x[None, i:i + block]
        dens += np.exp(-d * d / (2.0 * bw * bw)).sum(axis=1)
    return support, dens / (n * bw * np.sqrt(2.0 * np.pi)), (x.mean(), sd, bw)


def check_curve(got_support, got_density, want_support, want_density, tag=""):
    """support rtol 1e-12; density rtol 1e-9 plus atol 1e-12 x the peak.  Both sides are fp64: a sum of at most 44 162
    non-negative terms is off by about 5e-12 relative at most, a relative error of 1e-15 in bw moves a contributing term by
    about 36 x that; ddof = 0 moves the curve by about 1e-6, a wrong cut or factor by more."""
    got_support, got_density = np.asarray(got_support), np.asarray(got_density)
    assert got_support.shape == want_support.shape and got_density.shape == want_density.shape, tag
    assert got_support.dtype == np.float64 and got_density.dtype == np.float64, tag
    assert np.isfinite(want_density).all() and np.isfinite(got_density).all() and np.isfinite(got_support).all(), tag
    assert np.all(np.abs(got_support - want_support) <= 1e-12 * np.abs(want_support)), (tag, np.abs(got_support - want_support).max())
    err = np.abs(got_density - want_density)
    assert np.all(err <= 1e-9 * np.abs(want_density) + 1e-12 * want_density.max()), (tag, (err / want_density.max()).max())
