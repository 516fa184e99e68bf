"""CPU side of the bit-exact tests of the two output heads: K1c (csrc/head.hip, the generator's two 1x1 heads writing the
25 planes of the propagation step) and K1p (csrc/head1.hip, the plain 3x3 one-channel head).  Operands are small
integers, so that every product, every partial sum in any order and every stored result is an integer the number formats
hold exactly: fp32 FMA chains and fp32-accumulating MFMA below 2^24, one bf16 store of integers up to 256, fp32 partial
sums folded in fp64.  The comparison with plain torch on the CPU therefore needs no tolerance.

  head_case / head1_case    operands + references of one (shape, width, form); fp64, and where cheap int64 and fp32 as well
  preconditions             the conditions under which "exact" is a theorem, asserted by computation
  head_groups_per_sweep, head_grid_rows, head_trips    K1c's grid rule, stated once
  MUTANTS, old_criteria     one planted fault each, and what the tolerance tests of test_head_planes_gpu.py /
                            test_plain_head_gpu.py assert, restated
  *_view                    4-D views for assert_exact whose histograms are the kernels' own coordinates

No GPU import here: tests/test_heads_exact_cpu.py runs all of it on a machine without one.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tests.conv_exact_ref import LIMIT_ACC, LIMIT_BF16, _seed, assert_exact, int_tensor  # noqa: F401  (re-exported)

AMP = 3                        # |operand| <= AMP in the random forms
NP = 25                        # K1c planes
WPB = 4                        # K1c waves per workgroup (head.hip)
HEAD_MAX_WGS = 4096            # K1c's grid cap = rows of its workspace
CHEAP_MACS = 5e7               # references below this many multiply-adds are also taken in int64 and fp32
FILL = 7.0                     # what every result buffer holds before the launch
DTYPES = ("f32", "bf16")

LAUNCH_NAMES = ("head_forward", "head_backward", "head_dbias_fold", "head1_forward", "head1_backward", "head1_backward_fold")

# ------------------------------------------------------------------------------------------------------------------
# K1c: the grid rule
# ------------------------------------------------------------------------------------------------------------------


def head_grid_rows(groups: int, cus: int, per_cu: int = 4) -> int:
    """Workgroups head.hip's head_grid launches for `groups` 32-pixel groups: one wave per group up to per_cu workgroups
    per CU, at most 4096, at least one (JSPSR_HEAD_WGS=0 is therefore a single workgroup)."""
    return max(1, min((groups + WPB - 1) // WPB, cus * per_cu, HEAD_MAX_WGS))


def head_groups_per_sweep(cus: int, per_cu: int = 4) -> int:
    """Groups one trip of the grid-stride loop covers when the grid is at its cap: a raster with more takes a second trip."""
    return WPB * max(1, min(cus * per_cu, HEAD_MAX_WGS))


def head_trips(groups: int, rows: int) -> list:
    """Trips of the grid-stride loop per wave, wave-major (wave w of workgroup g is entry WPB g + w)."""
    n = rows * WPB
    return [len(range(w, groups, n)) for w in range(n)]


def two_trip_shape(cus: int, per_cu: int = 4):
    """(B, H, W) of 32 (groups per sweep + 64) pixels: 64 waves take a second trip.  (1, 260, 512) on a 256-CU part."""
    g = head_groups_per_sweep(cus, per_cu) + 64
    assert (g * 32) % 512 == 0
    return (1, g * 32 // 512, 512)


# ------------------------------------------------------------------------------------------------------------------
# K1c: cases
# ------------------------------------------------------------------------------------------------------------------
K1C_SHAPES = [
    (1, 4, 8),         # one group, three idle waves
    (1, 4, 16),        # two groups
    (5, 2, 16),        # every group its own image
    (3, 4, 24),        # a workgroup's waves in two images
    (1, 32, 5),        # odd W
    (2, 8, 36),
]
K1C_CINS = (32, 64, 128)
K1C_FORMS = ("random", "onehot")
X_COFF, X_EXTRA = 8, 24        # the sliced forward: channels [8, 8 + Cin) of Cin + 24
DX_COFF, DX_EXTRA = 16, 24     # the data gradient: channels [16, 16 + Cin) of Cin + 24
ONE_WG_ENV = {"JSPSR_HEAD_WGS": "0"}
ONE_WG_SHAPES = [(2, 8, 36), (1, 4, 8)]      # one workgroup: trips 5, 5, 4, 4 across an image boundary; 1, 0, 0, 0


def onehot_channel(p: torch.Tensor, cin: int) -> torch.Tensor:
    """c(p) of the forward probe: walks all channels (3 is coprime to every width), shifted by one per 32-pixel group."""
    return (3 * p + p // 32) % cin


def onehot_plane(p: torch.Tensor) -> torch.Tensor:
    """n(p) of the backward probe: walks all 25 planes, shifted by one per group."""
    return (7 * p + p // 32) % NP


def _mm(a, b):
    return a @ b


@functools.lru_cache(maxsize=4)
def head_case(shape, cin: int, form: str) -> dict:
    """x (B,H,W,Cin), w (25,Cin), b (25), g (B,25,H,W) and planes, dx, gn (B,H,W,32), db (25), dW (25,Cin): fp32 tensors of
    integers.  The tensors are shared between tests: nobody writes to them."""
    B, H, W = shape
    M = B * H * W
    gen = torch.Generator().manual_seed(_seed(f"k1c{shape}{cin}{form}"))
    bias = torch.arange(NP, dtype=torch.float32) - 12          # distinct per plane
    if form == "random":
        x = int_tensor(gen, (M, cin), AMP, 1.0)
        w = int_tensor(gen, (NP, cin), AMP, 1.0)
        g = int_tensor(gen, (B, NP, H * W), AMP, 1.0)
    elif form == "onehot":
        # forward: planes[n][p] = w[n][c(p)] + b[n], and w[n][c] = (c + n) % Cin - Cin/2 names c; backward: dx[p] = w[n(p)]
        p = torch.arange(M)
        x = torch.zeros(M, cin)
        x[p, onehot_channel(p, cin)] = 1
        n, c = torch.arange(NP).view(-1, 1), torch.arange(cin).view(1, -1)
        w = ((c + n) % cin - cin // 2).float()
        g = torch.zeros(B, H * W, NP)
        g.view(M, NP)[p, onehot_plane(p)] = 1
        g = g.permute(0, 2, 1).contiguous()
    else:
        raise ValueError(form)
    gm = g.permute(0, 2, 1).reshape(M, NP)                     # (pixels, planes)

    def ref(cast):
        xx, ww, gg, bb = cast(x), cast(w), cast(gm), cast(bias)
        return {"planes": _mm(xx, ww.t()) + bb, "dx": _mm(gg, ww), "db": gg.sum(0), "dW": _mm(gg.t(), xx)}

    r64 = ref(lambda t: t.double())
    c = {"kind": "k1c", "shape": shape, "cin": cin, "form": form, "x": x.view(B, H, W, cin), "w": w, "b": bias,
         "g": g.view(B, NP, H, W), "alt": {}}
    if float(M) * cin * NP <= CHEAP_MACS:
        c["alt"] = {"int64": ref(lambda t: t.long()), "fp32": ref(lambda t: t)}
    c["planes"] = r64["planes"].float().view(B, H * W, NP).permute(0, 2, 1).reshape(B, NP, H, W).contiguous()
    c["dx"] = r64["dx"].float().view(B, H, W, cin)
    c["gn"] = F.pad(gm, (0, 32 - NP)).view(B, H, W, 32)
    c["db"], c["dW"] = r64["db"].float(), r64["dW"].float()
    c["ref64"] = r64
    return c


def wide(t: torch.Tensor, coff: int, extra: int, seed: int) -> torch.Tensor:
    """(B,H,W,C) -> (B,H,W,C + extra) holding t in channels [coff, coff + C) and other integers beside it (a read outside the
    slice changes the result)."""
    gen = torch.Generator().manual_seed(seed)
    out = int_tensor(gen, tuple(t.shape[:3]) + (t.shape[3] + extra,), AMP, 1.0)
    out[..., coff:coff + t.shape[3]] = t
    return out


# ------------------------------------------------------------------------------------------------------------------
# K1p: cases
# ------------------------------------------------------------------------------------------------------------------
K1P_CS = (8, 24, 40, 72, 200, 248, 256)
K1P_TABLE = [
    ((1, 1, 1), K1P_CS),
    ((2, 7, 63), K1P_CS),
    ((1, 8, 64), K1P_CS),
    ((1, 9, 65), K1P_CS),
    ((1, 33, 65), K1P_CS),         # four backward tiles, halos both ways
    ((3, 17, 5), K1P_CS),
    ((1, 9, 255), (8, 24)),
    ((1, 9, 256), (8, 24)),
    ((1, 9, 257), (8, 24)),        # forward column blocks side by side
    ((1, 40, 130), (72,)),         # several tiles and bands at an odd chunk count
]
K1P_COFF, K1P_EXTRA = 8, 16        # x and dx: channels [8, 8 + C) of C + 16
FROWS, TROWS, TCOLS = 8, 32, 64    # head1.hip: forward band, backward tile
# where the deltas go (y, x): the two sides of a band edge, of a tile corner, of the forward's column-block seam
DELTA_AT = [(0, 0), (7, 63), (8, 64), (31, 63), (32, 64), (7, 255), (8, 256)]


def k1p_shapes(C: int) -> list:
    return [s for s, cs in K1P_TABLE if C in cs]


def delta_points(shape) -> list:
    """The points of DELTA_AT that lie in the raster, and its last pixel."""
    _, H, W = shape
    pts = [(y, x) for y, x in DELTA_AT if y < H and x < W]
    return pts + ([(H - 1, W - 1)] if (H - 1, W - 1) not in pts else [])


def k1p_forms(shape) -> list:
    return ["random"] + [f"delta@{y},{x}" for y, x in delta_points(shape)]


def k1p_tiles(shape) -> int:
    B, H, W = shape
    return B * ((H + TROWS - 1) // TROWS) * ((W + TCOLS - 1) // TCOLS)


def _conv_ref(x, w, b, dy):
    """F.conv2d and its autograd, in the dtype of the operands (NCHW)."""
    x, w, b = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = F.conv2d(x, w, b, 1, 1)
    y.backward(dy)
    return {"y": y.detach(), "dx": x.grad, "dW": w.grad, "db": b.grad}


def _taps_ref(x, w, b, dy):
    """The same four results from the nine shifted products, in int64 (NCHW in, NCHW out): no convolution routine, no
    autograd, another summation order."""
    x, w, b, dy = x.long(), w.long(), b.long(), dy.long()
    B, C, H, W = x.shape
    xp, gp = F.pad(x, (1, 1, 1, 1)), F.pad(dy, (1, 1, 1, 1))
    y = torch.zeros(B, 1, H, W, dtype=torch.long) + b.view(1, 1, 1, 1)
    dx = torch.zeros_like(x)
    dW = torch.zeros_like(w)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, ky:ky + H, kx:kx + W]                                   # x(y + ky - 1, x + kx - 1)
            y += (xs * w[0, :, ky, kx].view(1, C, 1, 1)).sum(1, keepdim=True)
            dW[0, :, ky, kx] = (xs * dy).sum((0, 2, 3))
            gs = gp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]                   # dy(y - ky + 1, x - kx + 1)
            dx += gs * w[0, :, ky, kx].view(1, C, 1, 1)
    return {"y": y, "dx": dx, "dW": dW, "db": dy.sum().view(1)}


@functools.lru_cache(maxsize=4)
def head1_case(shape, C: int, form: str) -> dict:
    """x (B,H,W,C), w (1,C,3,3), b (1), dy (B,1,H,W) and y (B,1,H,W), dx (B,H,W,C), dW (1,C,3,3), db (1)."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(_seed(f"k1p{shape}{C}"))
    w = int_tensor(gen, (1, C, 3, 3), AMP, 1.0)
    b = torch.tensor([5.0])
    if form == "random":
        x = int_tensor(gen, (B, C, H, W), AMP, 1.0)
        dy = int_tensor(gen, (B, 1, H, W), AMP, 1.0)
    elif form.startswith("delta@"):
        # y is the flipped 3x3 footprint of channel c around the point, dx the footprint of every channel, dW a single 1
        py, px = (int(v) for v in form[6:].split(","))
        x, dy = torch.zeros(B, C, H, W), torch.zeros(B, 1, H, W)
        x[B - 1, (py + px) % C, py, px] = 1
        dy[B - 1, 0, py, px] = 1
    else:
        raise ValueError(form)
    r64 = _conv_ref(x.double(), w.double(), b.double(), dy.double())
    c = {"kind": "k1p", "shape": shape, "C": C, "form": form, "x": x.permute(0, 2, 3, 1).contiguous(), "x_nchw": x, "w": w,
         "b": b, "dy": dy, "ref64": r64, "alt": {}}
    if float(B) * H * W * C * 9 <= CHEAP_MACS:
        c["alt"] = {"int64": _taps_ref(x, w, b, dy), "fp32": _conv_ref(x, w, b, dy)}
    c["y"] = r64["y"].float()
    c["dx"] = r64["dx"].float().permute(0, 2, 3, 1).contiguous()
    c["dW"], c["db"] = r64["dW"].float(), r64["db"].float()
    return c


# ------------------------------------------------------------------------------------------------------------------
# conditions
# ------------------------------------------------------------------------------------------------------------------

def _is_int(t) -> bool:
    return bool(torch.equal(t, t.round()))


def preconditions(c: dict, dtype: str) -> None:
    """Every stored operand is an integer of magnitude <= 256 (a bf16 number, hence also an fp32 one), every result stored in
    bf16 is, and no partial sum -- bounded by count x max x max, whatever the order -- reaches 2^24.  AssertionError, never
    a skip."""
    assert dtype in DTYPES
    tag = f"{c['kind']}{c['shape']}/{c.get('cin', c.get('C'))}/{c['form']}/{dtype}"
    mx = lambda t: t.abs().max().item()
    B, H, W = c["shape"]
    M = B * H * W
    if c["kind"] == "k1c":
        operands, K = ("x", "w", "b", "g"), c["cin"]
        sums = {"planes": K * mx(c["x"]) * mx(c["w"]) + mx(c["b"]), "dx": NP * mx(c["g"]) * mx(c["w"]),
                "db": M * mx(c["g"]), "dW": M * mx(c["g"]) * mx(c["x"])}
        stored = ("dx", "gn")
        results = ("planes", "dx", "gn", "db", "dW")
        assert (H * W) % 32 == 0 and K in K1C_CINS, tag
    else:
        operands, K = ("x", "w", "b", "dy"), c["C"]
        sums = {"y": 9 * K * mx(c["x"]) * mx(c["w"]) + mx(c["b"]), "dx": 9 * mx(c["dy"]) * mx(c["w"]),
                "db": M * mx(c["dy"]), "dW": M * mx(c["dy"]) * mx(c["x"])}
        stored = ("dx",)
        results = ("y", "dx", "db", "dW")
        assert K % 8 == 0 and 0 < K <= 256, tag
    for k in operands:
        assert _is_int(c[k]) and mx(c[k]) <= LIMIT_BF16, (tag, k, "is not an integer tensor within +-256")
        assert torch.equal(c[k].bfloat16().float(), c[k]), (tag, k, "is not a bf16 tensor")
    for k, v in sums.items():
        assert v < LIMIT_ACC, (tag, k, "partial sums can reach", v)
    for k in results:
        assert _is_int(c[k]) and mx(c[k]) < LIMIT_ACC, (tag, k)
        assert torch.equal(c[k].double().flatten(), _flat64(c, k)), (tag, k, "fp32 does not hold the fp64 reference")
    if dtype == "bf16":
        for k in stored:
            assert mx(c[k]) <= LIMIT_BF16, (tag, k, "max |stored| is", mx(c[k]))
            assert torch.equal(c[k].bfloat16().float(), c[k]), (tag, k, "a stored value is not a bf16 number")


def _flat64(c, k):
    """The fp64 reference of result k in the element order of c[k]."""
    B, H, W = c["shape"]
    if c["kind"] == "k1c":
        if k == "gn":
            return c["gn"].double().flatten()
        r = c["ref64"][k]
        return r.view(B, H * W, NP).permute(0, 2, 1).flatten() if k == "planes" else r.flatten()
    r = c["ref64"][k]
    return r.permute(0, 2, 3, 1).flatten() if k == "dx" else r.flatten()


def references_agree(c: dict) -> int:
    """fp64, int64 and fp32 references bit for bit (the result does not depend on the summation order); returns how many
    alternative references were compared."""
    for name, alt in c["alt"].items():
        for k, v in alt.items():
            assert torch.equal(v.double(), c["ref64"][k]), (c["kind"], c["shape"], c["form"], name, k)
    return len(c["alt"])


# ------------------------------------------------------------------------------------------------------------------
# views for assert_exact: the histograms are the kernels' coordinates
# ------------------------------------------------------------------------------------------------------------------
PLANES_AXES, PLANES_HISTS = ("b", "plane", "group in image", "pixel in group"), ((3, None), (1, None), (2, None), (0, None))
PIX_AXES, PIX_HISTS = ("group", "pixel in group", "channel half", "c in half"), ((1, None), (2, None), (3, 16), (0, None))
ROW_AXES, ROW_HISTS = ("-", "-", "n", "c"), ((2, None), (3, 16))
K1P_AXES, K1P_HISTS = ("b", "y", "x", "c"), ((1, 32), (2, 64), (1, 8), (3, 8), (0, None))     # tile row / column, band row, chunk lane


def planes_view(t):
    """(B,25,H,W) -> (B, 25, groups per image, 32)."""
    return t.reshape(t.shape[0], NP, -1, 32)


def pix_view(t):
    """NHWC (B,H,W,C) -> (groups, 32, 2, C/2): pixel in its 32-pixel group, the lane half h, the channel inside the half."""
    C = t.shape[3]
    return t.reshape(-1, 32, 2, C // 2)


def row_view(t):
    """(25,Cin) / (1,C,3,3) / (n,) -> 4-D (1, 1, rows, columns)."""
    t = t.reshape(t.shape[0], -1) if t.dim() == 2 else (t.reshape(t.shape[1], 9) if t.dim() == 4 else t.reshape(1, -1))
    return t.reshape(1, 1, *t.shape)


def y_view(t):
    """(B,1,H,W) -> (B,H,W,1)."""
    return t.permute(0, 2, 3, 1)


def check(got, want, what, view):
    """assert_exact at zero tolerance through one of the views above."""
    axes, hists = {planes_view: (PLANES_AXES, PLANES_HISTS), pix_view: (PIX_AXES, PIX_HISTS), row_view: (ROW_AXES, ROW_HISTS),
                   y_view: (K1P_AXES, K1P_HISTS), None: (K1P_AXES, K1P_HISTS)}[view]
    v = view or (lambda t: t)
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert_exact(v(got.detach().cpu().float()), v(want), what, axes=axes, hists=hists, edge=view in (y_view, None))


# ------------------------------------------------------------------------------------------------------------------
# what the tolerance tests assert, restated
# ------------------------------------------------------------------------------------------------------------------

def old_criteria(got, ref, what: str, dtype: str = "f32", pixels: int = 1):
    """Would tests/test_head_planes_gpu.py / tests/test_plain_head_gpu.py accept `got` for `ref`?  True / False, or None
    where those files never look at the tensor at all (K1c's NHWC gradient copy; K1c's bytes beside a slice)."""
    if what in ("k1c_gn", "k1c_outside"):
        return None
    if what == "k1p_outside":
        return bool((got == FILL).all())
    g, r = got.double(), ref.double()
    err, top = (g - r).abs(), r.abs().max().item()
    if what in ("k1c_planes", "k1c_dx"):
        rel = 2.0 ** -8 if (what == "k1c_dx" and dtype == "bf16") else 1e-5
        return err.max().item() < rel * max(1.0, top)
    if what == "k1c_db":
        return err.max().item() < 1e-4 * pixels ** 0.5
    if what == "k1c_dW":
        return err.max().item() < 1e-4 * max(1.0, top)
    if what == "k1p_y":
        return err.max().item() <= 2e-6 * top + 1e-7
    if what == "k1p_dx":
        if dtype == "f32":
            return err.max().item() <= 1e-5 * top
        return bool((err <= 2.0 ** -8 * r.abs() + 1e-6 * top).all())
    if what in ("k1p_dW", "k1p_db"):
        return ((g - r).norm() / r.norm().clamp_min(1e-30)).item() <= 1e-5
    raise ValueError(what)


# ------------------------------------------------------------------------------------------------------------------
# mutants: one fault each, applied to the reference result
# ------------------------------------------------------------------------------------------------------------------
_M_K1C = ((2, 8, 36), 64, "random")
_M_K1P = ((1, 33, 65), 24, "random")


def _m_second_trip():
    """One workgroup (JSPSR_HEAD_WGS=0) on (2, 8, 36): wave 0's second trip is group 4; its 32 pixels stay unwritten."""
    c = head_case(*_M_K1C)
    assert head_trips(18, 1) == [5, 5, 4, 4]
    got = planes_view(c["planes"]).clone()
    got[0, :, 4] = 0
    return "k1c_planes", got.view_as(c["planes"]), c["planes"], planes_view


def _m_swap_planes():
    c = head_case(*_M_K1C)
    got = c["planes"].clone()
    got[:, [8, 9]] = got[:, [9, 8]]
    return "k1c_planes", got, c["planes"], planes_view


def _m_swap_halves():
    c = head_case(*_M_K1C)
    h = c["cin"] // 2
    return "k1c_dx", torch.cat((c["dx"][..., h:], c["dx"][..., :h]), 3), c["dx"], pix_view


def _m_gn_padding():
    c = head_case(*_M_K1C)
    got = c["gn"].clone()
    got[1, 7, 35, 29] = 1
    return "k1c_gn", got, c["gn"], pix_view


def _m_halo_column():
    """The tile at x0 = 64 stages no dy halo column (x = 63): pixel column 64 loses tap kx = 2 in dx and dW."""
    c = head1_case(*_M_K1P)
    x, w, dy = c["x_nchw"], c["w"], c["dy"]
    H = x.shape[2]
    gp = F.pad(dy, (0, 0, 1, 1))                                                  # rows -1 .. H
    dx, dW = c["dx"].clone(), c["dW"].clone()
    for ky in range(3):
        col = gp[:, 0, 2 - ky:2 - ky + H, 63]                                     # dy(y - ky + 1, 63), (B, H)
        dx[:, :, 64, :] -= col.unsqueeze(2) * w[0, :, ky, 2].view(1, 1, -1)
        dW[0, :, ky, 2] -= (x[:, :, :, 64] * col.unsqueeze(1)).sum((0, 2))
    return [("k1p_dx", dx, c["dx"], None), ("k1p_dW", dW, c["dW"], row_view)]


def _m_band_tap():
    """The first row of the second band (y = 8) loses tap ky = 0, the input row above it."""
    c = head1_case(*_M_K1P)
    x, w = c["x_nchw"], c["w"]
    row = F.pad(x[:, :, 7:8, :], (1, 1))                                          # input row 7, columns -1 .. W
    got = c["y"].clone()
    got[:, :, 8:9] -= F.conv2d(row, w[:, :, 0:1, :])
    return "k1p_y", got, c["y"], y_view


def _m_inactive_lanes():
    """C = 24: three chunks per pixel, 21 pixels per wave step, lane 63 idle.  A walk that steps by 22 pixels per wave
    leaves slot 21 of every 22 unprocessed: dx keeps its fill there, dW misses those pixels."""
    c = head1_case(*_M_K1P)
    assert c["C"] == 24 and 64 // (24 // 8) == 21
    B, H, W = c["shape"]
    i = torch.arange(TROWS * TCOLS)
    skip = ((i % (4 * 22)) % 22 == 21).view(TROWS, TCOLS)
    m = skip.repeat((H + TROWS - 1) // TROWS, (W + TCOLS - 1) // TCOLS)[:H, :W]    # (H, W), the same in every tile
    dx = c["dx"].clone()
    dx[:, m] = FILL
    xm = c["x_nchw"] * (~m).float()
    dW = _conv_ref(xm.double(), c["w"].double(), c["b"].double(), c["dy"].double())["dW"].float()
    return [("k1p_dx", dx, c["dx"], None), ("k1p_dW", dW, c["dW"], row_view)]


def _m_outside_slice(kind):
    def make():
        c = head_case(*_M_K1C) if kind == "k1c" else head1_case(*_M_K1P)
        beside = torch.full(tuple(c["dx"].shape[:3]) + (DX_EXTRA if kind == "k1c" else K1P_EXTRA,), FILL)
        got = beside.clone()
        got[0, 1, 2, 3] = 1.0
        return f"{kind}_outside", got, beside, None
    return make


def _m_fold_row(kind):
    def make():
        if kind == "k1c":        # default grid on (2, 8, 36): 5 workgroups, the last one holds groups 16 and 17
            c = head_case(*_M_K1C)
            assert head_grid_rows(18, 256) == 5
            last = planes_view(c["g"])[1, :, 7:9].sum((1, 2))      # groups 16, 17 = groups 7, 8 of image 1
            return "k1c_db", c["db"] - last, c["db"], row_view
        c = head1_case(*_M_K1P)  # four tiles: the last one is rows 32.., columns 64..
        return "k1p_db", c["db"] - c["dy"][0, 0, 32:, 64:].sum(), c["db"], row_view
    return make


# name -> (maker, does a case of the two tolerance files reach the place the fault sits in?)
MUTANTS = {
    "k1c: second-trip group left unwritten": (_m_second_trip, "only the model-scale test (2x256x512), under 1e-4 / 1e-2"),
    "k1c: planes 8 and 9 swapped": (_m_swap_planes, "yes"),
    "k1c: dx channel halves swapped": (_m_swap_halves, "yes"),
    "k1c: non-zero in gn channel 25..31": (_m_gn_padding, "no: gn is consumed as [:25]"),
    "k1c: one element beside the dx slice": (_m_outside_slice("k1c"), "no: dx is always dense"),
    "k1c: last partial row of the db fold dropped": (_m_fold_row("k1c"), "yes"),
    "k1p: dy halo column of the tile at x0 = 64 dropped": (_m_halo_column, "only 256x512, C in (8, 64, 256)"),
    "k1p: tap ky = 0 dropped at band row y = 8": (_m_band_tap, "37x61 and 256x512"),
    "k1p: C = 24 inactive-lane walk skips pixels": (_m_inactive_lanes, "only the C = 24 autograd test, one shape"),
    "k1p: one element beside the dx slice": (_m_outside_slice("k1p"), "yes"),
    "k1p: last partial row of the dW / db fold dropped": (_m_fold_row("k1p"), "yes"),
}


def run_mutant(name):
    """-> [(what, got, want, view)]: the faulty results of one mutant."""
    out = MUTANTS[name][0]()
    return out if isinstance(out, list) else [out]
