"""TEST INFRASTRUCTURE ONLY -- planted cases, fp64 references and the yardstick for K1 (prop.hip, prop_dma.hip), its logits
entry (jspsr_prop_logits_*) and K1h (prop_head.hip, prop_head_dma.hip).

Every offset is a multiple of 2^-10 with |offset| < 2048, so the sampling position pixel + tap + offset is the same number
in fp32 and in fp64: kernel and oracle stand on the same side of every kink, and no kink mask is needed anywhere.  On top of
a random bulk (sigma 2 px) `case` plants taps of the classes below (CLASSES) and returns one boolean mask per class.

Reference: oracle.jspsr_ref.propagate and propagate_analytic_backward (the closed form: torchvision's per-corner rule, no
`inside` gate on the coordinate derivative -- what the kernels implement), in fp64; the same two functions in fp32 give the
floor that sets the tolerance (`atol`).  Autograd of `propagate` is NOT the reference: it gates the whole sample and so
differs from the closed form on the lines p = -1 (tests/test_prop_planted_cpu.py keeps that difference pinned).
"""
import numpy as np
import torch

from oracle import jspsr_ref as R

Q = 2.0 ** -10                       # every offset is a multiple of this
OFF_MAX = 2048.0
HALO = 8                             # prop_tile.h
TILES = {"dma": (4, 64), "general": (8, 64)}      # prop_dma.h (NW = 4 rows x DW = 64) / prop.hip's default tile
FAR = 1.0e6                          # what the oracle gets for a non-finite / 3e9 offset: far outside every raster
EPS32 = 2.0 ** -23
RTOL = 1e-5
RTOL_BF16 = 2.0 ** -8                # half a bf16 ulp is 2^-9; x 2 for fp32 error that moves a value across a rounding tie
SIG_DELTA = 2.0 ** -21               # 8 fp32 ulp: the affinity disturbance that widens the yardstick of the sigmoid entries
CAPS = dict(out=2e-5, grad_weight=2e-5, grad_offset=2e-5, grad_wk=5e-4, grad_b0=5e-4)
QUANT = ("out", "grad_weight", "grad_offset", "grad_wk", "grad_b0")
CLASSES = ("K", "Ky", "Kx", "E", "HB", "OH", "L8", "L9", "FI", "FO", "X")
PER_CLASS = 36                       # taps planted per class where the raster has room (the census asks for 32)
TAP_ORDER = (0, 8, 4, 1, 2, 3, 5, 6, 7)           # the i-th tap of the j-th class goes to tap TAP_ORDER[(i + j) % 9] (% 8 without the centre)
KY = [k // 3 - 1 for k in range(9)]
KX = [k % 3 - 1 for k in range(9)]
SPECIALS = (float("inf"), float("-inf"), float("nan"), 3.0e9)

# The shapes of the GPU table (tests/test_prop_planted_gpu.py); the CPU test holds every one of them to the census, the
# exact coordinates and the tolerance caps.
SHAPES = [
    (1, 4, 64),        # one DMA tile
    (2, 6, 132),       # idle waves, a ragged last column tile
    (1, 28, 196),      # 3 tiles each way: L8 / L9 / FI live here
    (3, 12, 72),       # a workgroup's run crosses images
    (2, 13, 70),       # general kernel, ragged
    (2, 5, 3),         # general kernel, tiny
    (1, 1, 1),
]
BIG = (1, 260, 1028)   # more tiles than workgroups: one case per entry
SCALES = (1.0, 0.7)


def seed_of(shape, oc, bf16=False):
    """(bf16: + 11.  With + 7 the 267 280 values of grad_out at BIG add up to -807 and the fp32 sum's own error, 1.4e-4,
    puts grad_b0's derived atol at 5.5e-4, past its cap; this stream gives 240 and 1.1e-4.  Chosen from the reference.)"""
    B, H, W = shape
    return 1000 * B + 10 * H + W + oc + (11 if bf16 else 0)


def scale_of(shape):
    """Each shape runs at one residual scale; the table alternates 1.0 and 0.7."""
    return SCALES[(SHAPES + [BIG]).index(shape) % 2]


def to16(off18):
    return torch.cat((off18[:, :8], off18[:, 10:]), 1)


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


class _Planter:
    """Draws (y, x, offset_y, offset_x) for tap k per class.  Positions are chosen near the pixel, so that the offsets
    stay small enough to be bf16 values too (FO aside, which is re-checked after rounding)."""

    def __init__(self, rs, H, W):
        self.rs, self.H, self.W = rs, H, W
        self.ylow = [y for y in range(H) if y % 8 < 4 and (y // 8) * 8 - 9 >= 0]
        self.yhigh = [y for y in range(H) if y % 8 >= 4 and (y // 8) * 8 + 7 + 9 <= H - 1]
        self.xlow = [x for x in range(W) if x % 64 < 6 and (x // 64) * 64 - 9 >= 0]
        self.xhigh = [x for x in range(W) if x % 64 >= 58 and (x // 64) * 64 + 63 + 9 <= W - 1]
        self.fi_x = [(x, s) for x in range(W) for s in (-1, 1)
                     if (x % 64 <= 9 and x - 62 >= 0 if s < 0 else x % 64 >= 53 and x + 63 <= W - 1)]
        self.fi_y = [(y, s) for y in range(H) for s in (-1, 1) if (y - 28 >= 0 if s < 0 else y + 29 <= H - 1)]

    def rint(self, lo, hi):
        return int(self.rs.randint(lo, hi + 1))

    def pick(self, seq):
        return seq[self.rs.randint(len(seq))]

    def frac(self):
        return (0.5, 0.25)[self.rs.randint(2)]

    def inside_int(self, base, dim, r=5):
        return float(self.rint(max(0, base - r), min(dim - 1, base + r)))

    def inside_frac(self, base, dim):
        return float(min(max(base, 0), max(dim - 2, 0))) + self.frac()

    def near_line(self, line, dim):
        return min(max(line + self.rint(-4, 4), 0), dim - 1)

    def applicable(self, cls):
        if cls in ("L8", "L9"):
            return bool(self.ylow or self.yhigh or self.xlow or self.xhigh) and self.H >= 3 and self.W >= 3
        if cls == "FI":
            return bool(self.fi_x or self.fi_y) and self.H >= 3 and self.W >= 3
        return True

    def draw(self, cls, i, k):
        """-> (y, x, oy, ox): pixel and the two offsets of tap k (None: keep the bulk's value of that component)."""
        H, W, rs = self.H, self.W, self.rs
        y, x = self.rint(0, H - 1), self.rint(0, W - 1)
        by = lambda: y + KY[k]
        bx = lambda: x + KX[k]
        if cls == "K":
            py, px = self.inside_int(by(), H), self.inside_int(bx(), W)
        elif cls == "Ky":
            py, px = self.inside_int(by(), H), self.inside_frac(bx(), W)
        elif cls == "Kx":
            py, px = self.inside_frac(by(), H), self.inside_int(bx(), W)
        elif cls == "E":
            v = i % 7
            other = (lambda b, d: self.inside_frac(b, d)) if (i // 7) % 2 == 0 else (lambda b, d: self.inside_int(b, d))
            if v < 3:
                line = (-1, H - 1, H)[v]
                y = self.near_line(line, H)
                py, px = float(line), other(bx(), W)
            elif v < 6:
                line = (-1, W - 1, W)[v - 3]
                x = self.near_line(line, W)
                py, px = other(by(), H), float(line)
            else:
                y, x = self.near_line(-1, H), self.near_line(-1, W)
                py, px = -1.0, -1.0
        elif cls == "HB":
            v = i % 6
            f = lambda: 0.25 * self.rint(1, 3)
            lo_y, hi_y, lo_x, hi_x = v in (0, 4), v in (1, 5), v in (2, 4), v in (3, 5)
            if lo_y or hi_y:
                y = self.near_line(-1 if lo_y else H - 1, H)
            if lo_x or hi_x:
                x = self.near_line(-1 if lo_x else W - 1, W)
            py = (-1 if lo_y else H - 1) + f() if (lo_y or hi_y) else self.inside_frac(by(), H)
            px = (-1 if lo_x else W - 1) + f() if (lo_x or hi_x) else self.inside_frac(bx(), W)
        elif cls == "OH":
            v = i % 4
            if v == 0:
                y = self.rint(0, min(4, H) - 1)
                py, px = -(1.25 + 0.25 * self.rint(0, 24)), self.inside_frac(bx(), W)
            elif v == 1:
                x = self.rint(0, min(64, W) - 1)
                py, px = self.inside_frac(by(), H), -(1.25 + 0.25 * self.rint(0, 24))
            elif v == 2:
                y = self.rint(((H - 1) // 4) * 4, H - 1)
                py, px = H + 0.25 * self.rint(1, 12), self.inside_frac(bx(), W)
            else:
                x = self.rint(((W - 1) // 64) * 64, W - 1)
                py, px = self.inside_frac(by(), H), W + 0.25 * self.rint(1, 12)
        elif cls in ("L8", "L9"):
            d = 8 if cls == "L8" else 9
            sides = [s for s, lst in enumerate((self.ylow, self.yhigh, self.xlow, self.xhigh)) if lst]
            s = sides[i % len(sides)]
            f = 0.25 * self.rint(0, 2)                         # 0: the kink on the edge of the window itself
            if s == 0:
                y = self.pick(self.ylow)
                py, px = (y // 8) * 8 - d + f, self.inside_frac(bx(), W)
            elif s == 1:
                y = self.pick(self.yhigh)
                py, px = (y // 8) * 8 + 7 + d - 1 + f, self.inside_frac(bx(), W)
            elif s == 2:
                x = self.pick(self.xlow)
                py, px = self.inside_frac(by(), H), (x // 64) * 64 - d + f
            else:
                x = self.pick(self.xhigh)
                py, px = self.inside_frac(by(), H), (x // 64) * 64 + 63 + d - 1 + f
        elif cls == "FI":
            axes = [a for a, lst in enumerate((self.fi_x, self.fi_y)) if lst]
            a = axes[i % len(axes)]
            d = self.rint(20, 60 if a == 0 else 26) + 0.25 * self.rint(0, 3)
            if a == 0:
                x, s = self.pick(self.fi_x)
                py, px = self.inside_frac(by(), H), bx() + s * d
            else:
                y, s = self.pick(self.fi_y)
                py, px = by() + s * d, self.inside_frac(bx(), W)
        elif cls == "FO":
            v = i % 3
            mag = lambda dim: (1 if rs.randint(2) else -1) * (self.rint(dim + 20, 2000) + 0.5 * self.rint(0, 1))
            return y, x, (mag(H) if v != 1 else None), (mag(W) if v != 0 else None)
        elif cls == "X":
            s, mode = SPECIALS[i % 4], (i // 4) % 3
            return y, x, (s if mode != 1 else None), (s if mode != 0 else None)
        else:
            raise KeyError(cls)
        return y, x, py - by(), px - bx()


def case(B, H, W, oc, seed, sigma=2.0, bf16=False, amp=1.0):
    """Seeded operands (numpy's frozen RandomState stream) of one propagation step, in fp32: `dem` in [0, amp), `weight` =
    sigmoid(N(0,1)) for the planar entries, `logits` (|l| <= 6) for the logits and head entries, `offset` (B,18,H,W) in
    torchvision's layout (centre pair zero and unplanted for oc = 16), `wk`, `b0`, `gout`, `pad` (what the seven unused
    channels of a K1h head hold), and `masks`: class -> (B,9,H,W) bool, plus `planted`, their union.  bf16: logits,
    offsets and pad are bf16 values (a multiple of 2^-10 rounded to 8 significant bits is still one)."""
    rs = np.random.RandomState(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    dem = f32(amp * rs.rand(B, 1, H, W))
    weight = f32(1.0 / (1.0 + np.exp(-rs.randn(B, 9, H, W))))
    logits = f32(np.clip(2.0 * rs.randn(B, 9, H, W), -6.0, 6.0))
    off = f32(np.round(sigma * rs.randn(B, 18, H, W) / Q) * Q)
    wk = f32(1 + 0.3 * rs.randn(9))
    b0 = f32(0.1 * rs.randn(1))
    gout = f32(rs.randn(B, 1, H, W))
    pad = f32(rs.randn(B, H, W, 7))
    if oc == 16:
        off[:, 8:10] = 0
    taps = [k for k in TAP_ORDER if oc == 18 or k != 4]
    total = B * len(taps) * H * W
    pl = _Planter(rs, H, W)
    classes = [c for c in CLASSES if pl.applicable(c)]
    budget = total // 4
    n_each = min(PER_CLASS, budget // len(classes))
    plan = [(c, n_each) for c in classes] if n_each else [(c, 1) for c in ("K", "X", "E", "FO")[:budget]]
    used = np.zeros((B, 9, H, W), dtype=bool)
    masks = {c: torch.zeros(B, 9, H, W, dtype=torch.bool) for c in CLASSES}
    for j, (cls, n) in enumerate(plan):
        for i in range(n):
            k = taps[(i + j) % len(taps)]
            for _ in range(64):
                b = int(rs.randint(B))
                y, x, oy, ox = pl.draw(cls, i, k)
                if not used[b, k, y, x]:
                    break
            else:
                continue
            used[b, k, y, x] = True
            masks[cls][b, k, y, x] = True
            if oy is not None:
                off[b, 2 * k, y, x] = oy
            if ox is not None:
                off[b, 2 * k + 1, y, x] = ox
    if bf16:
        logits, off, pad = bf16_round(logits), bf16_round(off), bf16_round(pad)
    return dict(dem=dem, weight=weight, logits=logits, offset=off, wk=wk, b0=b0, gout=gout, pad=pad, oc=oc, bf16=bf16,
                masks=masks, planted=torch.from_numpy(used), shape=(B, H, W))


# ---- geometry of a case, replayed in fp64 ------------------------------------------------------------------------------
def positions(off18, dtype=torch.float64):
    """(py, px), each (B,9,H,W), evaluated in `dtype` the way the kernels do: (pixel + tap) + offset."""
    B, _, H, W = off18.shape
    ys = torch.arange(H, dtype=dtype).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=dtype).view(1, 1, 1, W)
    ky = torch.tensor(KY, dtype=dtype).view(1, 9, 1, 1)
    kx = torch.tensor(KX, dtype=dtype).view(1, 9, 1, 1)
    o = off18.to(dtype).reshape(B, 9, 2, H, W)
    return (ys + ky) + o[:, :, 0], (xs + kx) + o[:, :, 1]


def special(off18):
    """(B,9,H,W): taps with a non-finite or |.| >= 2048 offset component (the X class)."""
    B, _, H, W = off18.shape
    return (~(off18.abs() < OFF_MAX)).reshape(B, 9, 2, H, W).any(2)


def all_corners_outside(off18):
    """(B,9,H,W): taps none of whose four corners is inside the raster (X taps included)."""
    B, _, H, W = off18.shape
    py, px = positions(oracle_offset(off18))
    fy, fx = py.floor(), px.floor()
    return (fy + 1 < 0) | (fy > H - 1) | (fx + 1 < 0) | (fx > W - 1)


def in_lds_window(off18, tile):
    """(B,9,H,W): the four corners come out of the staged tile + halo of the pixel's own tile (`inl` of prop_tile.h /
    prop_dma.h) for tiles of tile = (TH, TW) rows x columns."""
    B, _, H, W = off18.shape
    th, tw = tile
    py, px = positions(oracle_offset(off18))
    ry = py.floor() - ((torch.arange(H).view(1, 1, H, 1) // th) * th - HALO)
    rx = px.floor() - ((torch.arange(W).view(1, 1, 1, W) // tw) * tw - HALO)
    return (ry >= 0) & (ry < th + 2 * HALO - 1) & (rx >= 0) & (rx < tw + 2 * HALO - 1)


def oracle_offset(off18):
    """The offsets the oracle is given: X components (inf, NaN, 3e9) land far outside instead."""
    return torch.where(off18.abs() < OFF_MAX, off18, torch.full_like(off18, FAR))


def moved_outside(c):
    """A copy of the case whose taps without any corner inside the raster sample somewhere else outside it: every output of
    a kernel must have the same bits for both (such a tap contributes exactly nothing, wherever it is)."""
    off = c["offset"].clone()
    B, _, H, W = off.shape
    dead = all_corners_outside(off)
    if c["oc"] == 16:
        dead[:, 4] = False
    o = off.reshape(B, 9, 2, H, W)
    o[:, :, 0][dead] = -(H + 40.5)
    o[:, :, 1][dead] = W + 72.25
    return dict(c, offset=o.reshape(B, 18, H, W))


# ---- references ----------------------------------------------------------------------------------------------------------
def _oracle(c, affinity, scale, dtype):
    t = lambda a: a.to(dtype)
    off = t(oracle_offset(c["offset"]))
    wk, b0 = t(c["wk"]).reshape(1, 1, 3, 3), t(c["b0"])
    out = R.propagate(t(c["dem"]), affinity, off, wk, b0, scale)
    gw, go, gk, gb = R.propagate_analytic_backward(t(c["dem"]), affinity, off, wk, b0, t(c["gout"]))
    if c["oc"] == 16:
        go = to16(go)
    return dict(out=out, grad_weight=gw, grad_offset=go, grad_wk=gk.reshape(9), grad_b0=gb.reshape(1))


def planar_refs(c, scale):
    """(fp64, fp32) references of the planar entry: affinities as stored."""
    return _oracle(c, c["weight"].double(), scale, torch.float64), _oracle(c, c["weight"], scale, torch.float32)


def _logit_chain(r, a):
    r = dict(r)
    r["grad_weight"] = r["grad_weight"] * a * (1 - a)          # d/d(logit), by hand
    return r


def logits_refs(c, scale):
    """(fp64, fp32, allowance) of the entries that take logits (jspsr_prop_logits_*, K1h): a = sigmoid(logit) evaluated by
    the oracle, grad_weight = d/d(logit).  allowance: per quantity, max |fp64 oracle on a (1 + d) - fp64 oracle on a| with
    |d| = 2^-21 of random sign -- the kernels' sigmoid is v_rcp(1 + v_exp(-l log2 e)), not correctly rounded."""
    a64, a32 = torch.sigmoid(c["logits"].double()), torch.sigmoid(c["logits"])
    r64 = _logit_chain(_oracle(c, a64, scale, torch.float64), a64)
    r32 = _logit_chain(_oracle(c, a32, scale, torch.float32), a32)
    sign = torch.from_numpy(np.random.RandomState(12345).randint(0, 2, tuple(a64.shape)) * 2.0 - 1.0)
    ad = a64 * (1 + SIG_DELTA * sign)
    rd = _logit_chain(_oracle(c, ad, scale, torch.float64), ad)
    return r64, r32, {k: (rd[k] - r64[k]).abs().max().item() for k in QUANT}


def atol(r64, r32, extra=0.0):
    """The merged K1s rule: 4 x the fp32 reference's own error, floored at 4 ulp of the largest |ref| (+ the sigmoid
    allowance) -> (atol, fp32 floor)."""
    floor = (r32.double() - r64).abs().max().item() if r64.numel() else 0.0
    big = r64.abs().max().item() if r64.numel() else 0.0
    return max(4.0 * floor, 4.0 * EPS32 * big) + extra, floor


# ---- K1h's operand layout ------------------------------------------------------------------------------------------------
def pack_head(logits, off18, pad):
    """(B,9,H,W), (B,18,H,W), (B,H,W,7) -> the tap-major (B,H,W,32) head of prop_head.hip: channel 4 t + j of learned tap t
    (k = t < 4 ? t : t + 1) is j = 0 its logit, 1 dy, 2 dx, 3 the centre tap's logit for t = 0 and `pad` otherwise."""
    B, _, H, W = logits.shape
    h = torch.zeros(B, H, W, 8, 4, dtype=logits.dtype)
    for t in range(8):
        k = t if t < 4 else t + 1
        h[..., t, 0] = logits[:, k]
        h[..., t, 1] = off18[:, 2 * k]
        h[..., t, 2] = off18[:, 2 * k + 1]
    h[..., 0, 3] = logits[:, 4]
    h[..., 1:, 3] = pad.to(logits.dtype)
    return h.reshape(B, H, W, 32)


def unpack_head(h):
    """The inverse on a head gradient -> (grad_logit (B,9,H,W), grad_offset (B,16,H,W), pad (B,H,W,7))."""
    B, H, W, _ = h.shape
    h = h.reshape(B, H, W, 8, 4)
    lg = torch.stack([h[..., k if k < 4 else k - 1, 0] if k != 4 else h[..., 0, 3] for k in range(9)], 1)
    off = torch.stack([h[..., t, j] for t in range(8) for j in (1, 2)], 1)
    return lg, off, h[..., 1:, 3]
