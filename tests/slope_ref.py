"""numpy restatement of the slope-class plane (K22, jspsr_slope_classes), the yardstick of tests/test_slope_classes_gpu.py and
tests/test_strata_cpu.py.

`labels` is the kernel's arithmetic in numpy float32 operators, one rounding each, in the stated order, with
np.pad(mode="edge") per scene: the 3 x 3 taps a b c / d e f / g h i (a b c the row above),
    gx = ((c + 2f) + i) - ((a + 2d) + g);  gy = ((g + 2h) + i) - ((a + 2b) + c);  p = gx*gx + gy*gy,
the label the number of thresholds t_k <= p, 255 where any of the nine clamped taps is invalid or p is NaN.  numpy's
elementwise float32 operators do not contract, so every label is reproduced bit for bit.
`thresholds` is the formula in double, `degrees` the slope itself in float64 (what the thresholds stand for)."""
import math

import numpy as np


def thresholds(edges_deg, cell):
    return np.array([np.float32((8.0 * float(cell) * math.tan(float(e) * math.pi / 180.0)) ** 2) for e in edges_deg], dtype=np.float32)


def taps(z, dtype):
    t = np.pad(np.asarray(z, dtype=dtype), 1, mode="edge")
    h, w = np.asarray(z).shape
    return [[t[dy:dy + h, dx:dx + w] for dx in range(3)] for dy in range(3)]


def labels(z, thr, valid=None):
    """One scene: z (h, w) float32 metres, thr float32 thresholds, valid (h, w) bool / uint8 or None -> (h, w) uint8."""
    z = np.asarray(z)
    assert z.dtype == np.float32 and z.ndim == 2
    thr = np.asarray(thr, dtype=np.float32)
    (a, b, c), (d, _, f), (g, h, i) = taps(z, np.float32)
    two = np.float32(2.0)
    with np.errstate(all="ignore"):
        gx = ((c + two * f) + i) - ((a + two * d) + g)
        gy = ((g + two * h) + i) - ((a + two * b) + c)
        p = gx * gx + gy * gy
        assert p.dtype == np.float32
        lab = np.zeros(z.shape, dtype=np.int64)
        for t in thr:
            lab += t <= p
    lab[np.isnan(p)] = 255
    if valid is not None:
        ok = np.ones(z.shape, bool)
        for row in taps(np.asarray(valid) != 0, bool):
            for v in row:
                ok &= v
        lab[~ok] = 255
    return lab.astype(np.uint8)


def plane(scene_rasters, thr, valids=None):
    """A list of scenes -> the flat plane in store layout; no tap crosses a scene boundary because each scene is padded alone."""
    return np.concatenate([labels(z, thr, None if valids is None else valids[k]).reshape(-1) for k, z in enumerate(scene_rasters)])


def degrees(z, cell):
    """The slope in degrees, float64 throughout: atan(sqrt(gx^2 + gy^2) / (8 cell))."""
    (a, b, c), (d, _, f), (g, h, i) = taps(z, np.float64)
    gx = (c + 2 * f + i) - (a + 2 * d + g)
    gy = (g + 2 * h + i) - (a + 2 * b + c)
    return np.degrees(np.arctan(np.sqrt(gx * gx + gy * gy) / (8.0 * float(cell))))
