"""CPU side of the bit-exact convolution tests: integer operands for which every partial sum of the convolution is an
integer below 2^24, so that the fp32 accumulators of the MFMA kernels hold the exact result in any order and any split
over K or over pixels, and the comparison with torch's CPU convolution needs no tolerance.

  int_tensor      small integers times a Bernoulli mask
  ROWS / WROWS    the geometry tables: every row names the kernel(s) its launch must take
  forward_case / dgrad_case / wgrad_case   operands + reference of one (row, form)
  preconditions   the conditions under which "exact" is a theorem and the comparison sees (nearly) every element
  assert_exact    torch.equal with a diagnosis: where the mismatches are, by tile row / column / channel / image / edge

No GPU import here: tests/test_conv_exact_cpu.py runs all of it on a machine without one.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

LIMIT_ACC = float(2 ** 24)     # integers below it are exact in an fp32 accumulator
LIMIT_BF16 = 256.0             # every integer up to it is a bf16 number
FP64_MAX_MACS = 6e9            # references below this many multiply-adds are also taken in fp64 (about a second)
SCALES = (0.5, 1.0, 2.0, -1.0)
TARGET_VAR = 18.0 ** 2         # variance aimed at for a result element: max over 1e7 elements ~ 5.5 sigma ~ 100 < 256

P, P16, P16W, IG, R64, R128 = "conv_patch", "conv_patch_16x16", "conv_patch_16x16x128", "conv_igemm", "conv64_resident", "conv128_resident"
WG, WGP = "conv2d_wgrad", "conv2d_wgrad_patch"
CONV_KERNELS = (P, P16, P16W, IG, R64, R128)
WGRAD_KERNELS = (WG, WGP)
BOTH, F32, BF16 = ("f32", "bf16"), ("f32",), ("bf16",)

# fwd: x (B,H,W,Cin) -> (B,OH,OW,Cout).  dgrad ("same table"): the gathered gradient is (B,OH,OW,Cin), the written one
# (B,H,W,Cout) -- the data gradient of a conv Cout -> Cin on the H x W raster -- so that a row takes the same tile
# configuration in both directions.  `fwd` / `dgrad`: launches per kernel name the call must make, and no others (a stride-2
# data gradient is one launch per stride phase: the phases with more than one tap and a gathered channel count that is a
# multiple of the stage depth take the patch kernel, the single-tap phase the generic one).
Row = namedtuple("Row", "name B H W Cin Cout k stride pad dtypes fwd dgrad")

ROWS = [
    Row("patch_128x32", 2, 9, 21, 64, 24, 3, 1, 1, BOTH, {P: 1}, {P: 1}),            # ragged against 8x16, Cout % 8 != 0
    Row("patch_128x32_c96", 2, 12, 20, 96, 32, 3, 1, 1, F32, {P: 1}, {P: 1}),        # fp32 twin of igemm_c96
    Row("patch_128x64", 2, 17, 35, 64, 40, 3, 1, 1, BOTH, {P: 1}, {P: 1}),
    Row("patch_128x128_ntail", 1, 10, 18, 128, 136, 3, 1, 1, BOTH, {P: 1}, {P: 1}),
    Row("patch_128x128_deepk", 1, 8, 8, 1536, 256, 3, 1, 1, BOTH, {P: 1}, {P: 1}),
    Row("patch_16x16_f32", 4, 250, 255, 64, 64, 3, 1, 1, F32, {P16: 1}, {P16: 1}),   # exactly 1024 tiles, ragged both ways
    Row("patch_16x16_bf16", 4, 250, 255, 128, 48, 3, 1, 1, BF16, {P16: 1}, {P16: 1}),
    Row("patch_16x16_wide", 2, 250, 255, 64, 96, 3, 1, 1, BOTH, {P16: 1}, {P16: 1}),  # the Cout > 64 branch
    Row("igemm_3x3_s2", 1, 13, 17, 64, 72, 3, 2, 1, BOTH, {IG: 1}, {P: 3, IG: 1}),
    Row("igemm_1x1_s2", 2, 9, 11, 64, 128, 1, 2, 0, BOTH, {IG: 1}, {IG: 4}),         # three phases have no tap at all
    Row("igemm_head9", 1, 12, 12, 128, 9, 1, 1, 0, BOTH, {IG: 1}, {IG: 1}),
    Row("igemm_head16", 1, 12, 12, 128, 16, 1, 1, 0, BOTH, {IG: 1}, {IG: 1}),
    Row("igemm_head25", 1, 12, 12, 128, 25, 1, 1, 0, BOTH, {IG: 1}, {IG: 1}),
    Row("igemm_stem4", 2, 20, 20, 4, 32, 5, 1, 2, F32, {IG: 1}, {IG: 1}),
    Row("igemm_stem16", 1, 20, 28, 16, 32, 5, 1, 2, BOTH, {IG: 1}, {IG: 1}),
    Row("igemm_c96", 2, 12, 20, 96, 32, 3, 1, 1, BF16, {IG: 1}, {IG: 1}),            # Cin % 64 != 0
    Row("igemm_dbuf_24", 1, 12, 12, 192, 24, 3, 2, 1, BOTH, {IG: 1}, {P: 3, IG: 1}),  # K = 1728 > 1152: two LDS buffers
    Row("igemm_dbuf_48", 1, 12, 12, 192, 48, 3, 2, 1, BOTH, {IG: 1}, {P: 3, IG: 1}),
    Row("k2r_512_tiles", 2, 256, 256, 64, 64, 3, 1, 1, BF16, {R64: 1}, {R64: 1}),    # two tiles per workgroup
    Row("k2r_ragged", 3, 200, 216, 64, 64, 3, 1, 1, BF16, {R64: 1}, {R64: 1}),
    Row("k2q_2048_tiles", 2, 256, 512, 128, 128, 3, 1, 1, BF16, {R128: 1}, {R128: 1}),
]

# the transposed-convolution use of the data gradient: ConvTranspose2d k3 s2 p1 op1, (2, 12, 10, C) -> (2, 24, 20, C)
TCONV_ROWS = [Row(f"tconv_{c}", 2, 24, 20, c, c, 3, 2, 1, BOTH, None, {P: 3, IG: 1}) for c in (64, 256)]

# in_affine + input ReLU: the patch kernel only
AFFINE_ROWS = [
    Row("affine_64", 2, 16, 64, 64, 64, 3, 1, 1, BOTH, {P: 1}, None),
    Row("affine_128", 1, 19, 128, 128, 64, 3, 1, 1, BOTH, {P: 1}, None),
]

# child processes: the resident kernels at tiny rasters (JSPSR_CONV_RESIDENT_MIN=1 / JSPSR_CONV_RESIDENT128_MIN=1) and the
# 8-wave 256 x 128 tile (JSPSR_CONV_TALL=2)
_TINY = [(1, 5, 3), (1, 16, 16), (1, 17, 33), (5, 20, 72), (2, 40, 100)]     # (5, 20, 72): a workgroup's run crosses images
K2R_TINY_ROWS = [Row(f"k2r_{b}x{h}x{w}", b, h, w, 64, 64, 3, 1, 1, BF16, {R64: 1}, {R64: 1}) for b, h, w in _TINY]
K2Q_TINY_ROWS = [Row(f"k2q_{b}x{h}x{w}", b, h, w, 128, 128, 3, 1, 1, BF16, {R128: 1}, {R128: 1})
                 for b, h, w in _TINY + [(1, 8, 16), (1, 9, 17)]]
TALL2_ROWS = [Row("patch_16x16x128", 2, 250, 255, 64, 96, 3, 1, 1, BOTH, {P16W: 1}, {P16W: 1})]
CHILD_TABLES = {
    "k2r_tiny": ({"JSPSR_CONV_RESIDENT_MIN": "1"}, K2R_TINY_ROWS),
    "k2q_tiny": ({"JSPSR_CONV_RESIDENT128_MIN": "1"}, K2Q_TINY_ROWS),
    "tall2": ({"JSPSR_CONV_TALL": "2"}, TALL2_ROWS),
}

FWD_FORMS = ("plain", "stats", "bias_relu", "scale_bias_addend_relu", "slices")
DGRAD_FORMS = ("plain", "addend", "addend_relu")

# weight gradient: G (B,OH,OW,Cout padded to a 16-byte chunk), X (B,H,W,Cin) -> dW (Cout,Cin,k,k) fp32
WRow = namedtuple("WRow", "name B H W Cin Cout k stride pad dtypes kernel forms transposed")
_G = ("plain",)
_NINE = ("plain", "slices", "accumulate", "x_affine_relu")
WROWS = [WRow(r.name, r.B, r.H, r.W, r.Cin, r.Cout, r.k, r.stride, r.pad, r.dtypes, WG, _G, False) for r in ROWS
         if r.name in ("igemm_3x3_s2", "igemm_1x1_s2", "igemm_head9", "igemm_head16", "igemm_head25", "igemm_stem4",
                       "igemm_stem16", "igemm_dbuf_24", "igemm_dbuf_48")] + [
    WRow("wgrad_n200", 1, 17, 19, 8, 200, 3, 1, 1, BOTH, WG, _G, False),
    WRow("wgrad9_64", 2, 64, 64, 64, 64, 3, 1, 1, BOTH, WGP, _NINE, False),
    WRow("wgrad9_two_chunks", 1, 23, 128, 128, 64, 3, 1, 1, BOTH, WGP, _NINE, False),
    WRow("wgrad9_tails", 3, 9, 64, 96, 160, 3, 1, 1, BOTH, WGP, _NINE, False),
    WRow("wgrad9_short", 1, 5, 192, 40, 72, 3, 1, 1, BOTH, WGP, _NINE, False),
    # ConvTranspose2d weight (I=64, O=32, 3, 3), k3 s2 p1 op1: G = its input (2,12,10,64), X = the gradient of its output
    WRow("wgrad_transposed", 2, 24, 20, 32, 64, 3, 2, 1, BOTH, WG, _G, True),
]


def epc(dtype: str) -> int:
    return 4 if dtype == "f32" else 8


def out_hw(r):
    return (r.H + 2 * r.pad - r.k) // r.stride + 1, (r.W + 2 * r.pad - r.k) // r.stride + 1


def int_tensor(gen: torch.Generator, shape, amp: int, density: float) -> torch.Tensor:
    """Integers uniform in [-amp, amp] times a Bernoulli(density) mask, as fp32."""
    v = torch.randint(-amp, amp + 1, tuple(shape), generator=gen).to(torch.float32)
    return v * (torch.rand(tuple(shape), generator=gen) < density).to(torch.float32)


def _seed(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def _draw_pair(gen, shape_a, shape_w, K, a_eff=None):
    """Activations (or gradients) in [-2, 2] and weights in [-3, 3] ([-1, 1] for deep K) at densities chosen so that a result
    element has variance about TARGET_VAR: the activation density by the depth of the sum, the weight density from the
    measured mean square of the (transformed) activations.  Returns (a, w)."""
    da = 0.5 if K <= 256 else (0.25 if K <= 4096 else 0.125)
    a = int_tensor(gen, shape_a, 2, da)
    t = a if a_eff is None else a_eff(a)
    aw = 3 if K <= 4096 else 1
    ew2 = aw * (aw + 1) / 3.0                          # E[w^2] of the unmasked draw
    dw = min(1.0, TARGET_VAR / (K * float((t * t).mean()) * ew2))
    return a, int_tensor(gen, shape_w, aw, dw)


def _both_precisions(fn, macs, *ts):
    """fn(*ts) in fp32; where the case is small enough also in fp64, and then the two must agree bit for bit."""
    y = fn(*ts)
    if macs <= FP64_MAX_MACS:
        y64 = fn(*[t.double() for t in ts])
        assert torch.equal(y.double(), y64), "the fp32 CPU reference is not exact on these operands"
    return y


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _macs(r):
    oh, ow = out_hw(r)
    return float(r.B) * oh * ow * r.Cin * r.Cout * r.k * r.k


def has_fp64(r) -> bool:
    return _macs(r) <= FP64_MAX_MACS


def tile_rows(y, pairs=False):
    """(B,OH,OW,C) -> (B * ceil(OH/8) * ceil(OW/16), 2, C): sum y and sum y^2 over each 8x16-pixel tile, tiles numbered
    image-major, then tile row, then tile column (jspsr_conv2d_stats_rows).  pairs: the 16x16-pixel tiles of the patch
    kernel report under their upper half's number and write zeros to the lower half's row (conv.hip: stats_epilogue, r2)."""
    B, H, W, C = y.shape
    ty, tx = (H + 7) // 8, (W + 15) // 16

    def per_tile(t):
        t = F.pad(t, (0, 0, 0, tx * 16 - W, 0, ty * 8 - H))
        return t.reshape(B, ty, 8, tx, 16, C).double().sum((2, 4)).reshape(B * ty * tx, C)

    st = torch.stack((per_tile(y), per_tile(y * y)), 1)
    if pairs:
        st = st.reshape(B, ty, tx, 2, C)
        lower = st[:, 1::2].clone()
        st[:, 0:2 * lower.shape[1]:2] += lower
        st[:, 1::2] = 0
        st = st.reshape(B * ty * tx, 2, C)
    assert st.abs().max() < LIMIT_ACC
    return st.float()


def tile16_rows(y):
    """(B,OH,OW,C) -> (B, ceil(OH/16), ceil(OW/16), 2, C): sum y and sum y^2 over each 16x16-pixel tile, taken directly (not
    from the 8x16 rows): what the two rows of a 16x16 tile of the patch kernel must add up to."""
    B, H, W, C = y.shape
    ty, tx = (H + 15) // 16, (W + 15) // 16

    def per_tile(t):
        t = F.pad(t, (0, 0, 0, tx * 16 - W, 0, ty * 16 - H))
        return t.reshape(B, ty, 16, tx, 16, C).double().sum((2, 4))

    st = torch.stack((per_tile(y), per_tile(y * y)), 3)
    assert st.abs().max() < LIMIT_ACC
    return st.float()


def fold_rows16(st, B, H, W):
    """Statistics rows (B * ceil(H/8) * ceil(W/16), 2, C) -> (B, ceil(H/16), ceil(W/16), 2, C): the two 8x16 rows of each
    16x16 tile added (exact: integers below 2^24)."""
    ty, tx = (H + 7) // 8, (W + 15) // 16
    st = st.reshape(B, ty, tx, 2, -1)
    if ty % 2:
        st = torch.cat((st, torch.zeros_like(st[:, :1])), 1)
    return st[:, 0::2] + st[:, 1::2]


def pack_ref(w, mode, c_pad):
    """What jspsr_pack_weight must produce: (O,I,KH,KW) -> [O][KH][KW][c_pad] (mode 0) / [I][KH][KW][c_pad] (mode 1)."""
    t = w.permute(0, 2, 3, 1) if mode == 0 else w.permute(1, 2, 3, 0)
    return F.pad(t, (0, c_pad - t.shape[3])).contiguous()


# ------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------

def _row(name):
    for r in ROWS + TCONV_ROWS + AFFINE_ROWS + K2R_TINY_ROWS + K2Q_TINY_ROWS + TALL2_ROWS:
        if r.name == name:
            return r
    raise KeyError(name)


@functools.lru_cache(maxsize=3)
def _forward_base(name: str, affine: bool):
    r = _row(name)
    g = torch.Generator().manual_seed(_seed(r.name))
    K = r.Cin * r.k * r.k
    aff = None
    a_eff = None
    if affine:
        sc = torch.tensor(SCALES)[torch.randint(0, 4, (r.Cin,), generator=g)]
        sh = torch.randint(-1, 2, (r.Cin,), generator=g).float()
        aff = torch.stack((sc, sh)).contiguous()
        a_eff = lambda a: F.relu(a * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    x, w = _draw_pair(g, (r.B, r.Cin, r.H, r.W), (r.Cout, r.Cin, r.k, r.k), K, a_eff)
    xin = x if a_eff is None else a_eff(x)
    y = _both_precisions(lambda a, b: F.conv2d(a, b, None, r.stride, r.pad), _macs(r), xin, w)
    return {"x": _nhwc(x), "w": w, "y": _nhwc(y), "xin_nchw": xin, "aff": aff}


def forward_case(r, form: str) -> dict:
    """Operands (NHWC, fp32 values that are exact in either storage type) and the expected result of one forward form."""
    base = _forward_base(r.name, form == "in_affine_relu")
    g = torch.Generator().manual_seed(_seed(r.name + form))
    y = base["y"]
    c = {"kind": "fwd", "row": r, "form": form, "x": base["x"], "w": base["w"], "conv": y, "xin_nchw": base["xin_nchw"],
         "bias": None, "scale": None, "addend": None, "relu": False, "stats": None, "in_affine": base["aff"],
         "in_coff": 0, "out_coff": 0, "out_pitch": r.Cout, "pre_relu": y, "stored": [y], "want": y}
    if form == "stats":
        c["stats_pairs"] = bool(set(r.fwd) & {P16, P16W})
        c["stats"] = tile_rows(y, pairs=c["stats_pairs"])
        c["stats16"] = tile16_rows(y)
    elif form == "bias_relu":
        c["bias"] = int_tensor(g, (r.Cout,), 3, 1.0)
        c["relu"] = True
        c["pre_relu"] = y + c["bias"]
        c["want"] = F.relu(c["pre_relu"])
        c["stored"] = [c["want"]]
    elif form == "scale_bias_addend_relu":
        c["scale"] = torch.tensor(SCALES)[torch.randint(0, 4, (r.Cout,), generator=g)]
        c["bias"] = int_tensor(g, (r.Cout,), 3, 1.0)
        c["addend"] = int_tensor(g, tuple(y.shape), 3, 0.5)
        c["relu"] = True
        mid = y * c["scale"] + c["bias"]               # rounded to the storage type before the addend joins
        c["pre_relu"] = mid + c["addend"]
        c["want"] = F.relu(c["pre_relu"])
        c["stored"] = [mid, c["want"]]
    elif form == "slices":
        # the operand is channels [in_coff, in_coff + Cin) of a wider tensor whose other channels hold integers too (a read
        # outside the slice changes the result); the result goes to channels [out_coff, out_coff + Cout) of a tensor of 7s
        e = 8
        c["in_coff"] = e
        wide = int_tensor(g, (r.B, r.H, r.W, r.Cin + 3 * e), 2, 0.5)
        wide[..., e:e + r.Cin] = base["x"]
        c["x"] = wide
        c["out_coff"] = e
        c["out_pitch"] = (r.Cout + e - 1) // e * e + 2 * e
    elif form not in ("plain", "in_affine_relu"):
        raise ValueError(form)
    return c


# ------------------------------------------------------------------------------------------------------------------
# data gradient
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=3)
def _dgrad_base(name: str):
    r = _row(name)
    g = torch.Generator().manual_seed(_seed(r.name + "dgrad"))
    oh, ow = out_hw(r)
    Cg, Cw = r.Cin, r.Cout
    # a written pixel sums Cg * ceil(k / stride)^2 products
    K = Cg * ((r.k + r.stride - 1) // r.stride) ** 2
    go, w = _draw_pair(g, (r.B, Cg, oh, ow), (Cg, Cw, r.k, r.k), K)     # conv weight (O = Cg, I = Cw)
    oph = r.H - ((oh - 1) * r.stride - 2 * r.pad + r.k)
    opw = r.W - ((ow - 1) * r.stride - 2 * r.pad + r.k)
    dx = _both_precisions(lambda a, b: F.conv_transpose2d(a, b, None, r.stride, r.pad, (oph, opw)), _macs(r), go, w)
    assert dx.shape == (r.B, Cw, r.H, r.W)
    # pixels no tap reaches (1x1 stride 2: three of the four stride phases) are zeros by construction, not by chance
    reach = F.conv_transpose2d(torch.ones(1, 1, oh, ow), torch.ones(1, 1, r.k, r.k), None, r.stride, r.pad, (oph, opw)) > 0
    return {"g": _nhwc(go), "g_nchw": go, "w": w, "dx": _nhwc(dx), "op": (oph, opw), "reach": reach[0, 0]}


def dgrad_case(r, form: str) -> dict:
    base = _dgrad_base(r.name)
    g = torch.Generator().manual_seed(_seed(r.name + "dgrad" + form))
    dx = base["dx"]
    c = {"kind": "dgrad", "row": r, "form": form, "g": base["g"], "g_nchw": base["g_nchw"], "w": base["w"], "conv": dx,
         "op": base["op"], "reach": base["reach"], "addend": None, "relu": False, "pre_relu": dx, "stored": [dx], "want": dx, "bias": None,
         "scale": None}
    if form in ("addend", "addend_relu"):
        c["addend"] = int_tensor(g, tuple(dx.shape), 3, 0.5)
        c["pre_relu"] = dx + c["addend"]
        c["relu"] = form == "addend_relu"
        c["want"] = F.relu(c["pre_relu"]) if c["relu"] else c["pre_relu"]
        c["stored"] = [dx, c["want"]]
    elif form != "plain":
        raise ValueError(form)
    return c


# ------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------

def wgrad_case(r, form: str, dtype: str) -> dict:
    """G is channel-padded to the storage type's 16-byte chunk (the padding holds integers too: R = Cout rows are kept)."""
    g = torch.Generator().manual_seed(_seed(r.name + form))
    oh, ow = out_hw(r)
    M = r.B * oh * ow
    d = min(1.0, max(0.25, (48.0 / M) ** 0.5))
    x = int_tensor(g, (r.B, r.Cin, r.H, r.W), 2, d)
    go = int_tensor(g, (r.B, r.Cout, oh, ow), 2, d)
    c = {"kind": "wgrad", "row": r, "form": form, "x_affine": None, "init": None, "g_coff": 0, "x_coff": 0}
    xin = x
    if form == "x_affine_relu":
        sc = torch.tensor(SCALES)[torch.randint(0, 4, (r.Cin,), generator=g)]
        sh = torch.randint(0, 2, (r.Cin,), generator=g).float()      # (0.5 x - 1 <= 0 for every x: a dead channel, a zero column of dW)
        c["x_affine"] = torch.stack((sc, sh)).contiguous()
        xin = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))

    def ref(a, b):
        w0 = torch.zeros(r.Cout, r.Cin, r.k, r.k, dtype=a.dtype, requires_grad=True)
        if r.transposed:       # weight (I, O, kh, kw) of a ConvTranspose2d whose input is G and whose output gradient is X
            F.conv_transpose2d(b, w0, None, r.stride, r.pad, (r.H - ((oh - 1) * r.stride - 2 * r.pad + r.k),
                                                              r.W - ((ow - 1) * r.stride - 2 * r.pad + r.k))).backward(a)
        else:
            F.conv2d(a, w0, None, r.stride, r.pad).backward(b)
        return w0.grad

    dw = _both_precisions(ref, float(M) * r.Cin * r.Cout * r.k * r.k, xin, go)
    c["conv"] = dw
    c["abs"] = ref(xin.abs(), go.abs())
    c["want"] = dw
    e = epc(dtype)
    cgp = (r.Cout + e - 1) // e * e
    G = torch.cat((_nhwc(go), int_tensor(g, (r.B, oh, ow, cgp - r.Cout), 2, d)), 3) if cgp > r.Cout else _nhwc(go)
    X = _nhwc(x)
    if form == "slices":
        c["g_coff"], c["x_coff"] = 8, 16
        Gw = int_tensor(g, (r.B, oh, ow, cgp + 24), 2, d)
        Gw[..., 8:8 + cgp] = G
        Xw = int_tensor(g, (r.B, r.H, r.W, r.Cin + 24), 2, d)
        Xw[..., 16:16 + r.Cin] = X
        G, X = Gw, Xw
    elif form == "accumulate":
        c["init"] = int_tensor(g, tuple(dw.shape), 50, 1.0)
        c["want"] = dw + c["init"]
    c["G"], c["X"], c["cg"] = G, X, cgp
    return c


# ------------------------------------------------------------------------------------------------------------------
# conditions and comparison
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _abs_bound(name: str, kind: str, affine: bool) -> float:
    """max of conv(|x|, |w|): no partial sum of the convolution, in any order, exceeds it."""
    r = _row(name)
    if kind == "fwd":
        b = _forward_base(name, affine)
        return F.conv2d(b["xin_nchw"].abs(), b["w"].abs(), None, r.stride, r.pad).max().item()
    b = _dgrad_base(name)
    return F.conv_transpose2d(b["g_nchw"].abs(), b["w"].abs(), None, r.stride, r.pad, b["op"]).max().item()


def preconditions(c: dict, dtype: str) -> None:
    """The conditions under which the comparison is exact and sees the whole tensor.  A case that breaks one is a broken
    case: AssertionError, never a skip."""
    r, tag = c["row"], f"{c['row'].name}/{c['form']}/{dtype}"
    if c["kind"] == "wgrad":
        bound = c["abs"].abs().max().item() + (c["init"].abs().max().item() if c["init"] is not None else 0.0)
        assert bound < LIMIT_ACC, (tag, "partial sums can reach", bound)
        nz = (c["conv"] != 0).float().mean().item()
        assert nz >= 0.90, (tag, "non-zero share of the reference", nz)
        return
    bound = _abs_bound(r.name, c["kind"], c["form"] == "in_affine_relu") * (c["scale"].abs().max().item() if c["scale"] is not None else 1.0)
    bound += c["bias"].abs().max().item() if c["bias"] is not None else 0.0
    bound += c["addend"].abs().max().item() if c["addend"] is not None else 0.0
    assert bound < LIMIT_ACC, (tag, "partial sums can reach", bound)
    if dtype == "bf16":
        for t in c["stored"]:
            assert t.abs().max().item() <= LIMIT_BF16, (tag, "max |stored| is", t.abs().max().item())
            assert torch.equal(t.bfloat16().float(), t), (tag, "a stored value is not a bf16 number")
    if c.get("stats") is not None:
        assert c["stats"].abs().max().item() < LIMIT_ACC, tag
        sq = tile_rows(c["conv"].abs())
        assert sq.max().item() < LIMIT_ACC, tag
    pre = c["pre_relu"]
    if c["kind"] == "dgrad":       # the share is taken over the pixels a tap reaches; the others must come back as exact zeros
        pre = pre[:, c["reach"]]
    nz = (pre != 0).float().mean().item()
    assert nz >= 0.90, (tag, "non-zero share of the reference before ReLU", nz)
    if c["relu"]:
        lo, hi = (pre < 0).float().mean().item(), (pre > 0).float().mean().item()
        assert lo >= 0.25 and hi >= 0.25, (tag, "share clipped / passed by the ReLU", lo, hi)


def rel_fro(got, ref) -> float:
    """The criterion of the norm tests: ||got - ref|| / ||ref||."""
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30)).item()


ACT_HISTS = ((1, 16), (2, 16), (3, 64), (0, None))       # activations (b, y, x, c): by y % 16, x % 16, c % 64, image
WGRAD_AXES, WGRAD_HISTS = ("r", "c", "ky", "kx"), ((0, 64), (1, 64), (2, None), (3, None))
PACK_AXES, PACK_HISTS = ("n", "ky", "kx", "c"), ((0, 64), (1, None), (2, None), (3, 64))
STATS_AXES, STATS_HISTS = ("image * tile rows + tile row", "tile column", "sum|sumsq", "c"), ((0, None), (1, None), (2, None), (3, 64))


def stats_view(st, B, H, W):
    """Statistics rows (B * ty * tx, 2, C) as (B * ty, tx, 2, C) for assert_exact(axes=STATS_AXES, hists=STATS_HISTS)."""
    return st.reshape(B * ((H + 7) // 8), (W + 15) // 16, 2, -1)


def assert_exact(got: torch.Tensor, want: torch.Tensor, what: str, axes=("b", "y", "x", "c"), hists=ACT_HISTS, edge=None) -> None:
    """torch.equal on 4-D tensors.  On a mismatch the message carries the pattern: count, the first ten, and the mismatch
    counts along `hists` = ((axis, modulus or None), ...) -- for NHWC activations (the default) the histograms a
    tile-indexing bug shows up in, plus edge / interior of the raster; other tensors name their own axes and moduli."""
    edge = (hists is ACT_HISTS) if edge is None else edge
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    g32, w32 = got.to(torch.float32), want.to(torch.float32)
    bad = (g32 != w32) | torch.isnan(g32)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()
    lines = [f"{what}: {n} of {bad.numel()} elements differ ({axes[0]}, {axes[1]}, {axes[2]}, {axes[3]}, got, want):"]
    for i in idx[:10].tolist():
        lines.append(f"  ({i[0]}, {i[1]}, {i[2]}, {i[3]}, {g32[tuple(i)].item():g}, {w32[tuple(i)].item():g})")

    def hist(v, mod=None):
        v = v % mod if mod else v
        u, k = torch.unique(v, return_counts=True)
        return "{" + ", ".join(f"{a}: {b}" for a, b in zip(u.tolist(), k.tolist())) + "}"

    for ax, mod in hists:
        lines.append(f"  by {axes[ax]}{f' % {mod}' if mod else ''}: {hist(idx[:, ax], mod)}")
    if edge:
        B, H, W, C = bad.shape
        on = (idx[:, 1] == 0) | (idx[:, 1] == H - 1) | (idx[:, 2] == 0) | (idx[:, 2] == W - 1)
        lines.append(f"  on the edge of the {axes[1]}-{axes[2]} raster: {int(on.sum())}, interior: {n - int(on.sum())}")
    raise AssertionError("\n".join(lines))
