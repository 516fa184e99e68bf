"""numpy restatement of K25 (csrc/resample.hip): the axis taps in integers and double, the interpolation in float32 with
one rounding per operation, in the kernel's order.  The kernel's output has these bits."""
import numpy as np

f32 = np.float32
A = -0.75                                            # torch's and cv2.INTER_CUBIC's cubic convolution constant
NT = {"bicubic": 4, "bilinear": 2}                   # taps per axis
CENTRE = {"bicubic": 1, "bilinear": 0}               # the tap that is pixel i


def axis_taps(h, H, mode="bicubic"):
    """-> (first (H,) int32, weights (H, 4) float32): tap k of output Y is source index clip(first[Y] + k, 0, h - 1)."""
    if h < 1 or H < h:
        raise ValueError(f"{h} -> {H}")
    Y = np.arange(H, dtype=np.int64)
    n = (2 * Y + 1) * h - H
    d = np.int64(2 * H)
    if mode == "bilinear":
        n = np.maximum(n, 0)
    i = n // d                                        # floor, also below zero
    r = n - i * d
    t = r.astype(np.float64) / np.float64(d)
    w = np.zeros((H, 4), dtype=f32)
    if mode == "bilinear":
        w[:, 0] = (1.0 - t).astype(f32)
        w[:, 1] = t.astype(f32)
        return i.astype(np.int32), w
    c1 = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    c2 = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    w[:, 0] = c2(t + 1.0).astype(f32)
    w[:, 1] = c1(t).astype(f32)
    w[:, 2] = c1(1.0 - t).astype(f32)
    w[:, 3] = c2(2.0 - t).astype(f32)
    return (i - 1).astype(np.int32), w


def _taps(a, H, W, mode):
    """The gathered operands: v[k][j] (H, W) float32, the centre c, and the weights wy[k] (H, 1), wx[j] (1, W)."""
    h, w = a.shape
    nt, ct = NT[mode], CENTRE[mode]
    fy, wy = axis_taps(h, H, mode)
    fx, wx = axis_taps(w, W, mode)
    rows = [np.clip(fy.astype(np.int64) + k, 0, h - 1) for k in range(nt)]
    cols = [np.clip(fx.astype(np.int64) + j, 0, w - 1) for j in range(nt)]
    v = [[a[rows[k]][:, cols[j]] for j in range(nt)] for k in range(nt)]
    return v, v[ct][ct], [wy[:, k:k + 1] for k in range(nt)], [wx[None, :, j] for j in range(nt)]


def resample(a, H, W, mode="bicubic", clamp=None):
    """The kernel's arithmetic on one (h, w) float32 raster -> (H, W) float32."""
    a = np.ascontiguousarray(a, dtype=f32)
    nt = NT[mode]
    v, c, wy, wx = _taps(a, H, W, mode)
    with np.errstate(invalid="ignore", over="ignore"):
        r = []
        for k in range(nt):
            acc = (wx[0] * (v[k][0] - c).astype(f32)).astype(f32)
            for j in range(1, nt):
                acc = (acc + (wx[j] * (v[k][j] - c).astype(f32)).astype(f32)).astype(f32)
            r.append(acc)
        s = (wy[0] * r[0]).astype(f32)
        for k in range(1, nt):
            s = (s + (wy[k] * r[k]).astype(f32)).astype(f32)
        out = (s + c).astype(f32)
        if clamp is not None:
            lo, hi = f32(clamp[0]), f32(clamp[1])
            out = np.where(out < lo, lo, np.where(out > hi, hi, out)).astype(f32)
    return out


def slack(a, H, W, mode="bicubic"):
    """sum |wy_k wx_j| |v_kj - c| in float64: what the roundings of the interpolation scale with."""
    nt = NT[mode]
    v, c, wy, wx = _taps(np.ascontiguousarray(a, dtype=f32), H, W, mode)
    c = c.astype(np.float64)
    total = np.zeros((H, W), dtype=np.float64)
    for k in range(nt):
        for j in range(nt):
            total += np.abs(wy[k].astype(np.float64) * wx[j].astype(np.float64)) * np.abs(v[k][j].astype(np.float64) - c)
    return total


def tolerance(ref64, a, H, W, mode="bicubic"):
    """|out - ref| <= 2^-23 |ref| + 12 * 2^-24 * slack: the last rounding, and the longest path of roundings before it (one
    subtraction, two weight roundings, two products, six additions, one spare)."""
    return 2.0 ** -23 * np.abs(ref64) + 12 * 2.0 ** -24 * slack(a, H, W, mode)


def void_plane(v, H, W, mode="bicubic"):
    """The destination void plane: the source byte of pixel (clip(iy), clip(ix)), i the coordinate's floor."""
    h, w = v.shape
    ct = CENTRE[mode]
    fy, _ = axis_taps(h, H, mode)
    fx, _ = axis_taps(w, W, mode)
    return v[np.clip(fy.astype(np.int64) + ct, 0, h - 1)][:, np.clip(fx.astype(np.int64) + ct, 0, w - 1)]


def torch_ref(a, H, W, mode="bicubic"):
    """F.interpolate in float64 on the CPU -> (H, W) float64."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))[None, None]
    return F.interpolate(x, size=(H, W), mode=mode, align_corners=False)[0, 0].numpy()


def terrain(rng, h, w):
    """Elevations at 1500 m with 30 m of relief."""
    return (rng.random((h, w)) * 30 + 1500).astype(f32)
