"""CPU side of the exact tests of the per-channel kernels (K4/K5, csrc/elementwise.hip): operands on which the arithmetic
of BatchNorm forward / backward, ReLU / bias backward, the channel gate and the gate MLP is exact in fp32 in any order --
small integers, powers of two, a 1/16 offset that keeps every ReLU predicate away from zero -- with fp64 references, the
conditions under which "exact" is a theorem (`preconditions`), per-element bounds for the cases that cannot be exact
(batch statistics over a pixel count that is no power of two), the geometry tables, a mirror of the workspace layout and
the MUTANTS: corruptions of a correct result of the kind an indexing bug makes.

Layout: activations are (B, H, W, C) fp64 tensors holding values that are numbers of the storage type; parameters (C,).
`store(t, dt)` is what a kernel must leave in memory: the fp32 value, rounded to nearest even where the storage is bf16.

No GPU import here: tests/test_perchannel_exact_cpu.py runs all of it on a machine without one.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch

from tests.conv_exact_ref import LIMIT_ACC, _seed, assert_exact, int_tensor, rel_fro  # noqa: F401  (re-exported)

VEC = {"f32": 4, "bf16": 8}                  # channels per 16-byte lane group
TX, TY, PIX_FLY = 64, 4, 4                   # elementwise.hip: lanes per row, rows per workgroup, pixels in flight
U24, U8 = 2.0 ** -24, 2.0 ** -8
MOMENTUM = float(np.float32(0.1))            # the value the kernel sees
EPS_TRAIN = float(np.float32(1e-5))

# ------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------
# groups = C / vec:         1   3   5  16/8  48/24  64   65  384/192
CHANNELS = {"f32": (4, 12, 20, 64, 192, 256, 260, 1536),
            "bf16": (8, 24, 40, 64, 192, 512, 520, 1536)}
NARROW = {"f32": (4, 12, 20, 64), "bf16": (8, 24, 40, 64)}      # several pixels side by side in a 64-lane row
SLICE_WIDTHS = {"f32": (12, 64, 260), "bf16": (24, 64, 520)}    # operands at offset 32 inside a pitch of C + 64
SLICE_OFF, SLICE_PAD = 32, 64
R1, R35, R64, R198, R256, R4096 = (1, 1, 1), (1, 5, 7), (1, 8, 8), (2, 9, 11), (1, 16, 16), (1, 64, 64)

Geo = namedtuple("Geo", "dt C B H W")


def rasters(dt: str, C: int):
    """One chunk with the tail loop only, a power of two, several ragged chunks, several whole chunks; the 4096-pixel
    raster (main loop at wide C, 64 chunks) up to C = 256; the single pixel at the two widths where a ReLU share over
    C elements is still a statistic (C = 64 and 1536: at C = 4 it would be a share of four numbers)."""
    rs = [R35, R64, R198, R256]
    if C <= 256:
        rs.append(R4096)
    if C in (64, 1536):
        rs.append(R1)
    return rs


GEOS = [Geo(dt, C, *r) for dt in ("f32", "bf16") for C in CHANNELS[dt] for r in rasters(dt, C)]
# the child process (JSPSR_RED_BLOCKS=2): two chunks of 1250 pixels, the four-in-flight main loop at 64 pixels side by side
CHILD_ENV = {"JSPSR_RED_BLOCKS": "2"}
CHILD_GEOS = [Geo(dt, C, 1, 50, 50) for dt in ("f32", "bf16") for C in NARROW[dt]]
CHILD_TABLES = {"red_blocks_2": (CHILD_ENV, CHILD_GEOS)}

PARTIAL_ROWS = (1, 7, 256, 257, 300, 1000)          # bn_forward(partial=): copied up to 256 rows, folded above
EXT_ROWS = (1, 5, 1024, 1025, 1500)                 # bn_backward(ext_partial=): read in place up to 1024, folded above
MLP_SHAPES = ((1, 16, 1), (2, 72, 9), (2, 200, 12), (2, 80, 130), (1, 64, 257), (3, 1536, 96))      # (B, C, Ch)
WORKSPACE_EXTRA = {"f32": (1792, 2048), "bf16": (3584,)}


def geo_id(g: Geo) -> str:
    return f"{g.dt}-c{g.C}-{g.B}x{g.H}x{g.W}"


def make_red(npix: int, nseg: int, C: int, vec: int, target: int = 1024) -> dict:
    """elementwise.hip: make_red -- chunks per segment, pixels per chunk, lanes per pixel, pixels side by side."""
    gy = (C // vec + TX - 1) // TX
    want = max(1, target // (gy * nseg))
    chunks = max(1, min((npix + 63) // 64, want))
    chunk_pix = (npix + chunks - 1) // chunks
    chunks = (npix + chunk_pix - 1) // chunk_pix
    lpp = min(C // vec, TX)
    return {"gy": gy, "chunks": chunks, "chunk_pix": chunk_pix, "lpp": lpp, "pl": TX // lpp}


def main_loop_runs(npix: int, nseg: int, C: int, vec: int, target: int = 1024) -> bool:
    g = make_red(npix, nseg, C, vec, target)
    return (PIX_FLY - 1) * TY * g["pl"] < min(g["chunk_pix"], npix)


# ---- workspace: what is promised and what every entry point writes, in floats (include/jspsr_hip.h has the table) ----
FWD_EXT_ROWS = 256


def promised_floats(dt: str, C: int, nseg: int, target: int = 1024, parent: bool = False) -> int:
    """jspsr_reduce_workspace_bytes without its 64 spare bytes; parent=True: the formula before the forward's 256 external
    rows were counted."""
    rows = nseg * make_red(1 << 40, nseg, C, VEC[dt], target)["chunks"]
    planes = 3 * rows + 4
    return (planes if parent else max(planes, 2 + 2 * FWD_EXT_ROWS)) * C


def written_floats(entry: str, dt: str, C: int, nseg: int, npix: int, target: int = 1024, ext_rows: int = 0) -> int:
    ch = make_red(npix, nseg, C, VEC[dt], target)["chunks"]
    if entry == "bn_forward":                 # scale | shift, then [rows][2][C]
        return 2 * C + 2 * C * (min(ext_rows, FWD_EXT_ROWS) if ext_rows else ch)
    if entry == "bn_backward":                # coef [3][C], then [rows][2][C] (up to 1024 external rows are read in place)
        return 3 * C + 2 * C * ((min(ch, 1024) if ext_rows > 1024 else 0) if ext_rows else ch)
    if entry in ("act_backward", "gate_backward_reduce"):
        return nseg * ch * C
    if entry == "gate_pool":                  # sum | max | index
        return 3 * nseg * ch * C
    raise KeyError(entry)


# ------------------------------------------------------------------------------------------------------------------
# storage
# ------------------------------------------------------------------------------------------------------------------

def is_f32(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.float().double(), t.double()))


def is_stored(t: torch.Tensor, dt: str) -> bool:
    return is_f32(t) and (dt == "f32" or bool(torch.equal(t.float().bfloat16().double(), t.double())))


def store(t: torch.Tensor, dt: str) -> torch.Tensor:
    """The value a kernel leaves in memory for the exact fp32 result t: t itself, rounded to nearest even in bf16."""
    assert is_f32(t), "an exact result does not survive a float32 round trip"
    f = t.float()
    return f.bfloat16().float() if dt == "bf16" else f


def _gen(tag: str) -> torch.Generator:
    return torch.Generator().manual_seed(_seed(tag))


def _pow2(g, lo, hi, n):
    return 2.0 ** torch.randint(lo, hi + 1, (n,), generator=g).double()


def _sign(g, n):
    return torch.randint(0, 2, (n,), generator=g).double() * 2 - 1


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ------------------------------------------------------------------------------------------------------------------
# variant -> relu, residual, res_scale, res_affine, mask, slices
BN_VARIANTS = {
    "plain": (False, False, 1.0, False, False, False),
    "relu": (True, False, 1.0, False, False, False),
    "res": (False, True, 0.5, False, False, False),
    "res_relu_mask": (True, True, 1.0, False, True, False),
    "res_affine": (True, True, 0.5, True, True, False),
    "slice": (True, True, 0.5, False, True, True),
}


@functools.lru_cache(maxsize=4)
def bn_base(C: int, B: int, H: int, W: int) -> dict:
    """x, res, dy: integers in [-3, 3].  mean in {-1, 0, 1}, invstd in {1/4, 1/2, 1, 2} (running_var = 16, 4, 1, 1/4),
    gamma = +-{1/2, 1, 2}, beta = n + 1/16 with |n| <= 2 |gamma invstd| (so that the pre-activation changes sign inside the
    range of x on every channel, and is never zero: it is an odd multiple of 1/16 or 1/32)."""
    g = _gen(f"bn.{C}.{B}.{H}.{W}")
    sh = (B, H, W, C)
    b = {"C": C, "shape": sh, "npix": B * H * W}
    for k in ("x", "res", "dy"):
        b[k] = int_tensor(g, sh, 3, 0.9).double()
    b["invstd"] = _pow2(g, -2, 1, C)
    b["var"] = 1.0 / (b["invstd"] * b["invstd"])
    b["gamma"] = _sign(g, C) * _pow2(g, -1, 1, C)
    sc = (b["gamma"] * b["invstd"]).abs()
    nmax = torch.floor(2 * sc)
    b["beta"] = torch.floor(torch.rand(C, generator=g).double() * (2 * nmax + 1)) - nmax + 1.0 / 16
    b["mean"] = torch.randint(-1, 2, (C,), generator=g).double()
    # training mode normalises by the batch's own deviation (about 1.9 here): an offset of at most |gamma| / 2 keeps the
    # zero crossing inside the range of x
    b["beta_train"] = torch.sign(b["beta"] - 1.0 / 16) * b["gamma"].abs() / 2 + 1.0 / 16
    b["raff"] = torch.stack((_pow2(g, -1, 1, C), torch.randint(-1, 2, (C,), generator=g).double() / 2))     # res * {1/2, 1, 2} + {-1/2, 0, 1/2}
    b["acc0"] = torch.stack((int_tensor(g, (C,), 50, 1.0), int_tensor(g, (C,), 50, 1.0))).double()     # grads_into
    return b


def bn_eval_case(geo: Geo, variant: str) -> dict:
    """Eval mode, eps = 0: y, save_mean, save_invstd, the mask bytes, bn_fold and bn_reduce_params, all exact."""
    relu, res, rs, raff, mask, sl = BN_VARIANTS[variant]
    b = bn_base(*geo[1:])
    sc = b["gamma"] * b["invstd"]
    shf = b["beta"] - b["mean"] * sc
    bn = b["x"] * sc + shf
    terms = [b["x"] * sc, shf.expand_as(bn)]
    v = bn
    r = None
    if res:
        r = b["res"] * b["raff"][0] + b["raff"][1] if raff else b["res"]
        v = bn * rs + r
        terms = [t * rs for t in terms] + [r]
    y = store(torch.relu(v) if relu else v, geo.dt)
    c = dict(b, kind="bn_eval", geo=geo, variant=variant, relu=relu, with_res=res, res_scale=rs, with_raff=raff,
             want_mask=mask, sliced=sl, scale=sc, shift=shf, pre=v, y=y, save_mean=b["mean"].float(), save_invstd=b["invstd"].float(),
             inter=[sc, shf, bn, v] + ([r] if res else []), terms=terms,
             fold=((sc * rs).float(), (shf * rs).float()),
             red_par=torch.stack((sc, shf, b["invstd"], -b["mean"] * b["invstd"])).float())
    c["mask"] = mask_bytes(y, geo.dt)
    return c


def mask_bytes(y: torch.Tensor, dt: str) -> torch.Tensor:
    """[pixel][C / vec] bytes, bit k = (stored y of channel group * vec + k) > 0."""
    vec = VEC[dt]
    C = y.shape[-1]
    bits = (y.reshape(-1, C // vec, vec) > 0).to(torch.int64)
    return (bits << torch.arange(vec)).sum(-1).to(torch.uint8).reshape(-1)


def bn_train_case(geo: Geo, variant: str) -> dict:
    """Training mode: batch statistics.  save_mean is exact (integer sums, one double division, one cast); the rest is
    bounded: see bn_train_bound."""
    relu, res, rs, raff, mask, sl = BN_VARIANTS[variant]
    b = bn_base(*geo[1:])
    n = b["npix"]
    x2 = b["x"].reshape(n, -1)
    s, ss = x2.sum(0), (x2 * x2).sum(0)
    m = s / n
    var = (ss / n - m * m).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + EPS_TRAIN)
    sc = b["gamma"] * invstd
    t_x, t_b, t_m = b["x"] * sc, b["beta_train"].expand_as(b["x"]), (m * sc).expand_as(b["x"])
    v = t_x + t_b - t_m
    terms = [t_x, t_b, t_m]
    if res:
        r = b["res"] * b["raff"][0] + b["raff"][1] if raff else b["res"]
        v = v * rs + r
        terms = [t * rs for t in terms] + [r]
    rm0, rv0 = b["mean"], b["var"]
    unb = var * n / (n - 1) if n > 1 else var
    c = dict(b, kind="bn_train", geo=geo, beta=b["beta_train"], variant=variant, relu=relu, with_res=res, res_scale=rs, with_raff=raff,
             want_mask=mask, sliced=sl, sums=torch.stack((s, ss)), save_mean=m.float(), invstd64=invstd,
             rm64=(1 - MOMENTUM) * rm0 + MOMENTUM * m, rv64=(1 - MOMENTUM) * rv0 + MOMENTUM * unb,
             pre=v, y64=torch.relu(v) if relu else v, terms=terms)
    c["bound"] = elem_bound(terms, c["y64"], geo.dt)
    return c


def elem_bound(terms, ref, dt: str) -> torch.Tensor:
    """Per-element bound of an inexact fp32 evaluation: 8 * 2^-24 * sum |terms| (the terms with their outer factor already
    applied).  Derivation: the result is a sum of at most four terms, each the product of an operand that is exact and a
    per-channel coefficient that went through at most five fp32 roundings on its way (cast of the statistic, + eps, sqrt,
    division, the product with gamma or 1/npix), 2^-24 relative each; the products and additions of the expression itself
    round at 2^-24 of a magnitude that the sum of |terms| bounds, and there are at most three of them.  Five plus three,
    to first order: 8 * 2^-24 * sum |terms|.  ReLU is 1-Lipschitz, so the bound survives it.  A bf16 store adds half a
    bf16 ulp, at most 2^-8 |ref| -- plus 2^-8 of the fp32 error itself, which the factor (1 + 2^-8) carries."""
    e = 8 * U24 * sum(t.abs() for t in terms)
    if dt == "bf16":
        e = e * (1 + U8) + U8 * ref.abs()
    return e


def ulps32(got: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """|got - ref| in units of the fp32 ulp at ref."""
    ulp = 2.0 ** (torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -126))) - 23)
    return (got.double() - ref64).abs() / ulp


def partial_rows(c: dict, rows: int, scale: float = 1.0) -> torch.Tensor:
    """(rows, 2, C) fp32: integer rows (times `scale`) whose column sums are c['sums']."""
    g = _gen(f"rows.{rows}.{c['C']}")
    p = torch.randint(-5, 6, (rows, 2, c["C"]), generator=g).double() * scale
    p[-1] = c["sums"] - p[:-1].sum(0)
    assert p.abs().max() < LIMIT_ACC and is_f32(p) and torch.equal(p.sum(0), c["sums"])
    return p.float()


BWD_MODES = ("0", "0_dres", "1y", "1y_dres", "1m", "1m_dres", "2")     # relu mode and where the mask comes from; want_dres
_BWD_FWD = {"0": "plain", "0_dres": "res", "1y": "res_relu_mask", "1y_dres": "res_relu_mask", "1m": "res_relu_mask",
            "1m_dres": "res_relu_mask", "2": "relu"}


def bn_bwd_case(geo: Geo, mode: str, training: bool, dtype=torch.float64, perm=None, keep=None) -> dict:
    """dx, dres, dgamma, dbeta of the backward behind the eval-mode forward of _BWD_FWD[mode], with mean and invstd as
    given.  dtype / perm: the same expression evaluated in that type with the pixel sums taken in the order perm (the
    order-independence test); keep: a 0/1 weight per pixel inside the two sums (the dropped-pixel mutant)."""
    f = bn_eval_case(geo, _BWD_FWD[mode])
    n, C = f["npix"], f["C"]
    to = lambda t: t.to(dtype)
    dy, x = to(f["dy"]).reshape(n, C), to(f["x"]).reshape(n, C)
    mean, invstd, gamma, beta = to(f["mean"]), to(f["invstd"]), to(f["gamma"]), to(f["beta"])
    rs = f["res_scale"]
    xhat = (x - mean) * invstd
    if mode.startswith("0"):
        is_open = torch.ones_like(dy, dtype=torch.bool)
    elif mode == "2":
        is_open = gamma * xhat + beta > 0
        assert torch.equal(is_open, f["y"].reshape(n, C) > 0)
    else:
        is_open = f["y"].reshape(n, C) > 0
    dz = dy * is_open
    zx = dz * xhat
    order = torch.arange(n) if perm is None else perm
    w = torch.ones(n, 1, dtype=dtype) if keep is None else to(keep).reshape(n, 1)
    s, sx = (dz * w)[order].sum(0), (zx * w)[order].sum(0)
    k = gamma * invstd * rs
    exact = (not training) or (n & (n - 1)) == 0
    if training:
        a, bb = s.double() / n, sx.double() / n
        if dtype != torch.float64 or not exact:
            a, bb = a.float(), bb.float()                  # (float)(s / (double)count)
        a, bb = a.to(dtype), bb.to(dtype)
    else:
        a, bb = torch.zeros_like(s), torch.zeros_like(sx)
    t_a, t_b = a.expand_as(dz), xhat * bb
    dx = k * (dz - t_a - t_b)
    c = dict(kind="bn_bwd", geo=geo, C=C, mode=mode, training=training, fwd=f, exact=exact, want_dres="dres" in mode,
             relu=0 if mode.startswith("0") else (2 if mode == "2" else 1), open=is_open, dz=dz.reshape(f["shape"]),
             dbeta=s * rs, dgamma=sx * rs, dx=dx.reshape(f["shape"]), sums=torch.stack((s, sx)).double(),
             inter=[xhat, zx, s, sx, k, a, bb, dz - t_a, t_b, dx], abs_sums=torch.stack((dz.abs().sum(0), zx.abs().sum(0))))
    if not exact:
        # the reference keeps a, b in fp64; the kernel rounds them once each, which elem_bound's coefficient roundings cover
        a64, b64 = s.double() / n, sx.double() / n
        c["dx"] = (k * (dz - a64 - xhat * b64)).reshape(f["shape"])
        c["bound"] = elem_bound([k * dz, (k * a64).expand_as(dz), k * xhat * b64], c["dx"].reshape(n, C), geo.dt).reshape(f["shape"])
    return c


# ------------------------------------------------------------------------------------------------------------------
# ReLU / bias backward
# ------------------------------------------------------------------------------------------------------------------

def act_case(geo: Geo, relu: bool) -> dict:
    b = bn_base(*geo[1:])
    y = bn_eval_case(geo, "relu")["y"]          # a stored ReLU output with 20-80 % zeros
    dz = b["dy"] * (y > 0) if relu else b["dy"]
    return dict(kind="act", geo=geo, relu=relu, dy=b["dy"], y=y, dz=dz, dbias=dz.reshape(-1, b["C"]).sum(0), C=b["C"],
                abs_sums=dz.abs().reshape(-1, b["C"]).sum(0), open=y > 0)


# ------------------------------------------------------------------------------------------------------------------
# channel gate
# ------------------------------------------------------------------------------------------------------------------
GATE_FORMS = ("random", "ties", "negative")


def gate_geo(geo: Geo, B=None) -> tuple:
    """(B, npix, C) of the per-image kernels on a raster: (2, 9, 11) is two images of 99 pixels."""
    return (geo.B if B is None else B), geo.H * geo.W, geo.C


@functools.lru_cache(maxsize=4)
def gate_case(geo: Geo, form: str, B=None) -> dict:
    """x (B, npix, C) integers.  random: [-3, 3] (ties at the maximum occur by themselves, anywhere); ties: [-2, 2] with
    the value 3 planted at 2-4 pixels per (image, channel) -- pixel 0 and the last one, neighbours (another sub-lane or
    row of the workgroup), pixels half an image apart (another chunk), four at random; negative: [-3, -1]."""
    Bn, npix, C = gate_geo(geo, B)
    g = _gen(f"gate.{form}.{Bn}.{npix}.{C}")
    if form == "negative":
        x = torch.randint(-3, 0, (Bn, npix, C), generator=g).double()
    else:
        x = torch.randint(-3 if form == "random" else -2, (3 if form == "random" else 2) + 1, (Bn, npix, C), generator=g).double()
    if form == "ties":
        assert npix >= 4
        a = torch.randint(0, npix - 1, (Bn, C), generator=g)
        for b in range(Bn):
            for ch in range(C):
                p = int(a[b, ch])
                pix = ((0, npix - 1), (p, p + 1), (p // 2, p // 2 + npix // 2, npix - 1),
                       tuple(torch.randperm(npix, generator=g)[:4].tolist()))[(ch + b) % 4]
                x[b, list(pix), ch] = 3
    dy = torch.randint(-3, 4, (Bn, npix, C), generator=g).double()
    idx = torch.arange(Bn * C).reshape(Bn, C)
    s = (1.0 - 2.0 * ((idx // 7) % 2)) * 2.0 ** -(idx % 7).double()              # +-2^-k, k = 0..6
    davg = torch.randint(-3, 4, (Bn, C), generator=g).double()
    dmax = torch.randint(1, 4, (Bn, C), generator=g).double() * _sign(g, Bn * C).reshape(Bn, C)
    xn = x.numpy()
    amax = torch.from_numpy(np.argmax(xn, axis=1).astype(np.int32))              # first occurrence
    hit = torch.zeros_like(x)
    hit.scatter_(1, amax.long().unsqueeze(1), 1.0)
    c = dict(kind="gate", geo=geo, form=form, B=Bn, npix=npix, C=C, x=x, dy=dy, s=s, davg=davg, dmax=dmax,
             sum=x.sum(1), avg=torch.from_numpy((xn.sum(1) / np.float64(npix)).astype(np.float32)), mx=x.amax(1), amax=amax,
             n_max=(x == x.amax(1, keepdim=True)).sum(1), scaled=x * s.unsqueeze(1), ds=(dy * x).sum(1), hit=hit,
             abs_sums=torch.stack((x.abs().sum(1), (dy * x).abs().sum(1))))
    return c


def gate_apply_ref(c: dict, dt: str, davg=None) -> dict:
    """dx = dy s + davg / npix + [p == amax] dmax: exact where npix is a power of two or davg = 0, bounded otherwise."""
    davg = c["davg"] if davg is None else davg
    npix = c["npix"]
    t0, t1, t2 = c["dy"] * c["s"].unsqueeze(1), (davg / npix).unsqueeze(1).expand_as(c["dy"]), c["hit"] * c["dmax"].unsqueeze(1)
    dx = t0 + t1 + t2
    exact = (npix & (npix - 1)) == 0 or not bool(davg.any())
    out = {"dx": dx, "exact": exact, "inter": [t0, t1, t0 + t1, dx]}
    if not exact:
        # terms: dy s exact; davg / npix went through two roundings (1 / npix, the product); two additions
        out["bound"] = elem_bound([t0, t1, t2], dx, dt)
    return out


# ------------------------------------------------------------------------------------------------------------------
# gate MLP
# ------------------------------------------------------------------------------------------------------------------
MLP_S_LIMIT = 4 * U24       # two half-ulp roundings (1 + e, the division) of a value below 1, plus one ulp of expf


@functools.lru_cache(maxsize=None)
def mlp_case(B: int, C: int, Ch: int) -> dict:
    """Integer avg, mx, w1, w2, ds; sparse rows so that every sum is a small integer and the pre-sigmoid sum lies in
    [-8, 8].  The backward takes s as a dyadic number in {1/8, 1/4, 1/2, 3/4} (not the forward's s), so that
    ds s (1 - s) is a multiple of 1/64 and every gradient is exact."""
    g = _gen(f"mlp.{B}.{C}.{Ch}")
    avg = torch.randint(-2, 3, (B, C), generator=g).double()
    mx = torch.randint(-2, 3, (B, C), generator=g).double()
    w1 = int_tensor(g, (Ch, C), 1, min(1.0, 3.0 / C)).double()
    w1[torch.arange(Ch), torch.randint(0, C, (Ch,), generator=g)] = 1.0          # no empty row
    ha, hm = torch.relu(avg @ w1.T), torch.relu(mx @ w1.T)
    h = ha + hm
    # w2: up to eight candidate rows per channel (1-3 entries of +-1), the first whose sum stays in [-8, 8] for every
    # image; a row of zeros (s = 1/2) where none does
    w2 = torch.zeros(C, Ch, dtype=torch.float64)
    done = torch.zeros(C, dtype=torch.bool)
    for _ in range(8):
        cand = int_tensor(g, (C, Ch), 1, min(1.0, 2.0 / Ch)).double()
        cand[torch.arange(C), torch.randint(0, Ch, (C,), generator=g)] = _sign(g, C)
        ok = ((h @ cand.T).abs().amax(0) <= 8) & ~done
        w2[ok] = cand[ok]
        done |= ok
    z = h @ w2.T
    ds = torch.randint(-3, 4, (B, C), generator=g).double()
    s_in = torch.tensor([0.125, 0.25, 0.5, 0.75], dtype=torch.float64)[torch.randint(0, 4, (B, C), generator=g)]
    dz = ds * s_in * (1 - s_in)
    dh = dz @ w2                                       # (B, Ch)
    dha, dhm = dh * (ha > 0), dh * (hm > 0)
    return dict(kind="mlp", B=B, C=C, Ch=Ch, avg=avg, mx=mx, w1=w1, w2=w2, ds=ds, s_in=s_in, hid=torch.stack((ha, hm), 1), z=z,
                s=torch.sigmoid(z), dz=dz, davg=dha @ w1, dmax=dhm @ w1, dw1=dha.T @ avg + dhm.T @ mx, dw2=dz.T @ h,
                inter=[dz, dh], abs_sums=[avg.abs() @ w1.abs().T, h @ w2.abs().T, dz.abs() @ w2.abs(), dh.abs() @ w1.abs(),
                                          dh.abs().T @ (avg.abs() + mx.abs()), dz.abs().T @ h])


# ------------------------------------------------------------------------------------------------------------------
# conditions
# ------------------------------------------------------------------------------------------------------------------

def _share(is_open, tag):
    sh = is_open.double().mean().item()
    assert 0.2 <= sh <= 0.8, (tag, "share of open ReLUs", sh)


def preconditions(c: dict, dt: str) -> None:
    """The conditions under which the comparison of a case is exact (or its bound valid) and sees what it claims to see.
    A case that breaks one is a broken case: AssertionError, never a skip."""
    kind = c["kind"]
    tag = (kind, c.get("variant") or c.get("mode") or c.get("form"), dt, c.get("geo"))
    if kind in ("bn_eval", "bn_train"):
        for k in ("x", "res", "dy"):
            assert is_stored(c[k], dt), (tag, k, "is not a number of the storage type")
        for k in ("gamma", "beta", "mean", "var", "raff"):
            assert is_f32(c[k]), (tag, k)
        n = c["npix"]
        assert (c["x"].abs().reshape(n, -1).sum(0) < LIMIT_ACC).all() and ((c["x"] ** 2).reshape(n, -1).sum(0) < LIMIT_ACC).all(), tag
        if kind == "bn_eval":
            for t in c["inter"]:
                assert is_f32(t), (tag, "an intermediate does not survive a float32 round trip")
            assert torch.equal((1.0 / torch.sqrt(c["var"])).float().double(), c["invstd"]), tag
        if kind == "bn_eval" and c["relu"]:      # (training mode: the mask is checked against the kernel's own stored y)
            gap = c["pre"].abs().min().item()
            assert gap >= 1.0 / 32, (tag, "a pre-activation is within", gap, "of zero")
        if c["relu"]:
            _share(c["pre"] > 0, tag)
    elif kind == "bn_bwd":
        f = c["fwd"]
        preconditions(f, dt)
        assert (c["abs_sums"] * 4 < LIMIT_ACC).all(), (tag, "partial sums (in quarters) can reach 2^24")
        if c["exact"]:
            for t in c["inter"]:
                assert is_f32(t), (tag, "an intermediate does not survive a float32 round trip")
        if c["relu"]:
            _share(c["open"], tag)
        if c["mode"] == "2":
            assert (f["gamma"] * ((f["x"] - f["mean"]) * f["invstd"]) + f["beta"]).abs().min() >= 1.0 / 16, tag
    elif kind == "act":
        assert is_stored(c["dy"], dt) and is_stored(c["y"], dt), tag
        assert (c["abs_sums"] < LIMIT_ACC).all(), tag
        if c["relu"]:
            _share(c["open"], tag)
    elif kind == "gate":
        assert is_stored(c["x"], dt) and is_stored(c["dy"], dt) and is_stored(c["scaled"], dt), tag
        assert (c["abs_sums"] < LIMIT_ACC).all(), tag
        if c["form"] == "ties":
            assert (c["n_max"] >= 2).all(), (tag, "an (image, channel) without a tie at its maximum")
            assert (c["amax"] == 0).any() and (c["x"][:, -1] == c["mx"]).any(), (tag, "pixel 0 / the last pixel carry no maximum")
        if c["form"] == "negative":
            assert (c["mx"] < 0).all(), tag
        for zero_davg in (False, True):
            r = gate_apply_ref(c, dt, torch.zeros_like(c["davg"]) if zero_davg else None)
            if r["exact"]:
                for t in r["inter"]:
                    assert is_f32(t), (tag, "gate_backward_apply: an intermediate does not survive a float32 round trip")
    elif kind == "mlp":
        for k in ("avg", "mx", "w1", "w2", "ds", "hid", "davg", "dmax", "dw1", "dw2"):
            assert is_f32(c[k]), (tag, k)
        for t in c["inter"]:
            assert is_f32(t), tag
        z = c["z"]
        assert torch.equal(z, z.round()) and z.abs().max() <= 8, (tag, "pre-sigmoid sums", z.abs().max().item())
        assert z.unique().numel() >= (3 if c["Ch"] > 1 else 2), (tag, "the pre-sigmoid sums hardly vary")
        for t in c["abs_sums"]:
            assert (t * 64 < LIMIT_ACC).all(), (tag, "partial sums (in 64ths) can reach 2^24")
        assert (c["hid"] > 0).double().mean() >= 0.1 and c["dw1"].any() and c["dw2"].any() and c["davg"].any(), tag
    else:
        raise KeyError(kind)


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------

def as4(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    while t.dim() < 4:
        t = t.unsqueeze(0)
    return t


ROW_AXES, ROW_HISTS = ("-", "-", "row", "c"), ((2, None), (3, 64))
GATE_AXES, GATE_HISTS = ("-", "image", "pixel", "c"), ((1, None), (2, 64), (3, 64))


def check_exact(got, want, what, dt="f32", axes=None, hists=None):
    """assert_exact on tensors of any rank up to four; `want` is the exact fp64 value, compared as stored in dt."""
    w = want if want.dtype not in (torch.float64,) else store(want, dt)
    if got.dim() == 4 and axes is None:
        return assert_exact(got.float(), w.float(), what)
    if axes is None:
        axes, hists = (ROW_AXES, ROW_HISTS) if got.dim() <= 2 else (GATE_AXES, GATE_HISTS)
    assert_exact(as4(got).float(), as4(w).float(), what, axes=axes, hists=hists, edge=False)


def check_bound(got, ref64, bound, what):
    """|got - ref| <= bound per element; the message names the worst element and how many fail."""
    err = (got.detach().cpu().double() - ref64).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = torch.argmax(err - bound)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their bound; worst at flat index {int(i)}: "
                             f"error {err.flatten()[i].item():.3e}, bound {bound.flatten()[i].item():.3e}")


def old_criterion(got, ref, tol) -> tuple:
    """The relative-Frobenius criterion of tests/test_elementwise_gpu.py: (value, passes)."""
    v = rel_fro(got, ref)
    return v, v < tol


# ------------------------------------------------------------------------------------------------------------------
# mutants: a correct result, corrupted the way a kernel bug would
# ------------------------------------------------------------------------------------------------------------------

def _chunk_last_pixels(npix, C, dt, nseg=1):
    g = make_red(npix, nseg, C, VEC[dt])
    keep = torch.ones(npix)
    keep[torch.arange(g["chunks"]) * g["chunk_pix"] + g["chunk_pix"] - 1 if g["chunks"] * g["chunk_pix"] == npix else
         torch.cat((torch.arange(g["chunks"] - 1) * g["chunk_pix"] + g["chunk_pix"] - 1, torch.tensor([npix - 1])))] = 0
    return keep


def mut_drop_last_pixel_of_chunks(geo: Geo, mode: str, training: bool) -> dict:
    """BatchNorm backward whose reduce pass leaves the last pixel of every chunk out of both sums (p < p1 - 1)."""
    return bn_bwd_case(geo, mode, training, keep=_chunk_last_pixels(geo.B * geo.H * geo.W, geo.C, geo.dt))


def mut_swap_channels_in_group(t: torch.Tensor, dt: str) -> torch.Tensor:
    """Channels 1 and 2 of the last 16-byte group change places (a wrong index into the lane vector)."""
    t = t.clone()
    c0 = t.shape[-1] - VEC[dt]
    t[..., [c0 + 1, c0 + 2]] = t[..., [c0 + 2, c0 + 1]]
    return t


def mut_shift_lane_group(t: torch.Tensor, dt: str) -> torch.Tensor:
    """The first 16-byte channel group holds the values of the pixel before (a lane group that starts one pixel early)."""
    t = t.clone()
    flat = t.reshape(-1, t.shape[-1])
    flat[:, :VEC[dt]] = torch.roll(flat[:, :VEC[dt]], 1, 0)
    return flat.reshape(t.shape)


def mut_last_argmax(c: dict) -> torch.Tensor:
    """gate_pool taking the last maximal pixel (>= where > belongs)."""
    xn = c["x"].numpy()
    return torch.from_numpy((c["npix"] - 1 - np.argmax(xn[:, ::-1], axis=1)).astype(np.int32))


def mut_fold_drops_final_row(rows: torch.Tensor) -> torch.Tensor:
    """Column sums of the statistics rows without the final row (a fold loop that stops one row early)."""
    return rows[:-1].double().sum(0)


def mut_write_outside_slice(buf: torch.Tensor, off: int, C: int) -> torch.Tensor:
    """One element just past the slice [off, off + C) of the last pixel is overwritten."""
    buf = buf.clone()
    buf.reshape(-1, buf.shape[-1])[-1, off + C] = 0.0
    return buf


MUTANTS = {"drop_last_pixel_of_chunks": mut_drop_last_pixel_of_chunks, "swap_channels_in_group": mut_swap_channels_in_group,
           "shift_lane_group": mut_shift_lane_group, "last_argmax": mut_last_argmax, "fold_drops_final_row": mut_fold_drops_final_row,
           "write_outside_slice": mut_write_outside_slice}
