"""What tests/test_prop_planted_gpu.py stands on, checked without a GPU: the planted cases hold the classes they claim
(census and geometry, worked out from HALO and the 64 x 4 DMA tile / 64 x 8 general tile), every coordinate is exact in
fp32, the derived tolerances stay under their caps at every shape of the GPU table, the fp64 closed form agrees with the
plain-C oracle on the planted cases (kinks and the -1 lines included) and differs from autograd of `propagate` only on
the -1 lines -- so nobody swaps the reference later without this file noticing."""
import functools

import numpy as np
import pytest
import torch

from oracle import jspsr_ref as R
from oracle import prop_ref as C
from tests import prop_planted_ref as P

ALL = P.SHAPES + [P.BIG]
ID = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
# (oc, bf16): the operand sets of the GPU table -- planar 18 / 16, logits and fp32 head (oc 16), bf16 head
KINDS = [(18, False), (16, False), (16, True)]


@functools.lru_cache(maxsize=None)
def _case(shape, oc, bf16):
    return P.case(*shape, oc, P.seed_of(shape, oc, bf16), bf16=bf16)


def _large_enough(c):
    B, H, W = c["shape"]
    return (B * (9 if c["oc"] == 18 else 8) * H * W // 4) // len(P.CLASSES) >= 32


@pytest.mark.parametrize("oc,bf16", KINDS)
@pytest.mark.parametrize("shape", ALL, ids=ID)
def test_census_and_exact_coordinates(shape, oc, bf16):
    c = _case(shape, oc, bf16)
    B, H, W = shape
    off, m = c["offset"], c["masks"]
    x = P.special(off)
    fin = ~x.repeat_interleave(2, 1)                     # (B,18,H,W): components of non-X taps
    assert bool(((off[fin] / P.Q) == (off[fin] / P.Q).round()).all()) and bool((off[fin].abs() < P.OFF_MAX).all())
    assert torch.equal(x, m["X"])
    if bf16:
        assert torch.equal(P.bf16_round(off), off) or bool(torch.isnan(off).any())
        assert torch.equal(P.bf16_round(off).nan_to_num(7.0), off.nan_to_num(7.0))
    if oc == 16:
        assert bool((off[:, 8:10] == 0).all()) and not bool(c["planted"][:, 4].any())
    # every non-X coordinate is the same number in fp32 and fp64
    safe = torch.where(fin, off, torch.zeros_like(off))
    for p32, p64 in zip(P.positions(safe, torch.float32), P.positions(safe, torch.float64)):
        assert torch.equal(p32.double(), p64)
    # census
    n_taps = B * (9 if oc == 18 else 8) * H * W
    planted = sum(int(v.sum()) for v in m.values())
    assert planted == int(c["planted"].sum()) and 4 * planted <= n_taps, (planted, n_taps)
    print(f"  {shape} oc={oc} bf16={bf16}: " + " ".join(f"{k}={int(v.sum())}" for k, v in m.items()) + f"  planted {planted}/{n_taps}")
    if _large_enough(c):
        need = [k for k in P.CLASSES if k not in ("L8", "L9", "FI") or (H >= 24 and W >= 192)]
        for k in need:
            assert int(m[k].sum()) >= 32, (k, int(m[k].sum()))
            for tap in (0, 8) + ((4,) if oc == 18 else ()):
                assert bool(m[k][:, tap].any()), (k, tap)
    # geometry of every class, from the stored offsets
    py, px = P.positions(P.oracle_offset(off))
    fy, fx = py.floor(), px.floor()
    four_in = (fy >= 0) & (fy + 1 <= H - 1) & (fx >= 0) & (fx + 1 <= W - 1)
    dead = P.all_corners_outside(off)
    win = {k: P.in_lds_window(off, t) for k, t in P.TILES.items()}
    ys = torch.arange(H).view(1, 1, H, 1).expand(B, 9, H, W).double()
    xs = torch.arange(W).view(1, 1, 1, W).expand(B, 9, H, W).double()
    inty, intx = (py == fy) & (py >= 0) & (py <= H - 1), (px == fx) & (px >= 0) & (px <= W - 1)
    quarter = lambda p: ((p - p.floor()) == 0.5) | ((p - p.floor()) == 0.25)
    on = lambda p, d: (p == -1) | (p == d - 1) | (p == d)
    band = lambda p, d: ((p > -1) & (p < 0)) | ((p > d - 1) & (p < d))
    away = torch.maximum((py - ys).abs(), (px - xs).abs())
    ok = dict(K=inty & intx, Ky=inty & quarter(px), Kx=intx & quarter(py), E=on(py, H) | on(px, W),
              HB=band(py, H) | band(px, W), OH=dead & win["dma"] & win["general"], FO=dead & (away >= 19), X=x,
              FI=four_in & ~win["dma"] & ~win["general"] & (away >= 19) & (away <= 62))
    # L8 / L9: the last corner pair read from LDS and the first read by the global fallback, in BOTH tile geometries:
    # the window of a tile that starts at t0 and is T long holds floor(p) in [t0 - 8, t0 + T + 6]
    edge = {}
    for d in (8, 9):
        e = torch.zeros(B, 9, H, W, dtype=torch.bool)
        for th, tw in P.TILES.values():
            ty0, tx0 = (ys // th) * th, (xs // tw) * tw
            hit = (fy == ty0 - d) | (fy + 1 == ty0 + th - 1 + d) | (fx == tx0 - d) | (fx + 1 == tx0 + tw - 1 + d)
            e = hit if th == 4 else e & hit
        edge[d] = e
    ok["L8"] = four_in & win["dma"] & win["general"] & edge[8]
    ok["L9"] = four_in & ~win["dma"] & ~win["general"] & edge[9]
    for k in P.CLASSES:
        assert bool(ok[k][m[k]].all()), (k, int((~ok[k][m[k]]).sum()))
    assert bool((dead | ~(m["FO"] | m["X"])).all())


@pytest.mark.parametrize("shape", [(1, 28, 196), (2, 13, 70)], ids=ID)
def test_closed_form_matches_the_c_oracle(shape):
    """oracle/prop_ref.c in fp64 against propagate / propagate_analytic_backward on a planted case: 1e-12."""
    c = _case(shape, 18, False)
    r64, _ = P.planar_refs(c, 0.7)
    n = lambda t: t.double().numpy()
    off = n(P.oracle_offset(c["offset"]))
    out = C.forward(n(c["dem"]), n(c["weight"]), off, n(c["wk"]), float(c["b0"].double()[0]), 0.7)
    gw, go, gwk, gb = C.backward(n(c["gout"]), n(c["dem"]), n(c["weight"]), off, n(c["wk"]))
    for k, got in (("out", out), ("grad_weight", gw), ("grad_offset", go), ("grad_wk", gwk.reshape(9)), ("grad_b0", gb)):
        err = np.abs(got - r64[k].numpy()).max()
        print(f"  {k}: {err:.2e}")
        assert err <= 1e-12, (k, err)


def test_closed_form_and_autograd_differ_only_on_the_minus_one_lines():
    c = _case((1, 28, 196), 18, False)
    r64, _ = P.planar_refs(c, 1.0)
    t = lambda a: a.double()
    off = t(P.oracle_offset(c["offset"])).requires_grad_()
    out = R.propagate(t(c["dem"]), t(c["weight"]), off, t(c["wk"]).reshape(1, 1, 3, 3), t(c["b0"]), 1.0)
    out.backward(t(c["gout"]))
    py, px = P.positions(off.detach())
    line = ((py == -1) | (px == -1)).repeat_interleave(2, 1)
    diff = (off.grad - r64["grad_offset"]).abs()
    print(f"  on the -1 lines: {int(line.sum())} entries, max difference {diff[line].max().item():.3f}; off them {diff[~line].max().item():.1e}")
    assert int(line.sum()) >= 32 and diff[line].max().item() > 1e-2
    assert diff[~line].max().item() <= 1e-12
    assert bool((off.grad[line] == 0).all())              # autograd gates the whole sample there; the kernels do not


@pytest.mark.parametrize("shape", ALL, ids=ID)
def test_tolerance_caps(shape):
    """The derived atol of every quantity of every entry of the GPU table, at the scale the table uses."""
    scale = P.scale_of(shape)
    rows = []
    for oc in (18, 16):
        if shape == P.BIG and oc == 18:
            continue
        r64, r32 = P.planar_refs(_case(shape, oc, False), scale)
        rows.append((f"planar oc={oc}", r64, r32, dict.fromkeys(P.QUANT, 0.0)))
    for bf16 in (False, True):
        rows.append((f"logits bf16={bf16}",) + P.logits_refs(_case(shape, 16, bf16), scale))
    for what, r64, r32, extra in rows:
        for k in P.QUANT:
            a, floor = P.atol(r64[k], r32[k], extra[k])
            print(f"  {shape} {what} {k}: fp32 floor {floor:.2e} sigmoid allowance {extra[k]:.2e} atol {a:.2e} max|ref| {r64[k].abs().max().item():.2e}")
            assert a <= P.CAPS[k], (what, k, a)
            assert bool(torch.isfinite(r64[k]).all())


@pytest.mark.parametrize("shape", [(2, 6, 132), (2, 13, 70)], ids=ID)
def test_tolerance_caps_with_all_offsets_zero(shape):
    """The cases of test_all_offsets_zero (every tap on a kink in both components) meet the same caps."""
    scale = P.scale_of(shape)
    for oc, bf16 in KINDS:
        c = _case(shape, oc, bf16)
        c = dict(c, offset=torch.zeros_like(c["offset"]))
        for r64, r32, extra in (P.planar_refs(c, scale) + (dict.fromkeys(P.QUANT, 0.0),), P.logits_refs(c, scale)):
            assert r64["grad_offset"].abs().max().item() > 0.5          # the convention carries a real gradient here
            for k in P.QUANT:
                a, _ = P.atol(r64[k], r32[k], extra[k])
                assert a <= P.CAPS[k], (oc, bf16, k, a)


def test_head_layout_round_trip():
    c = _case((2, 5, 3), 16, True)
    h = P.pack_head(c["logits"], c["offset"], c["pad"])
    lg, off, pad = P.unpack_head(h)
    assert torch.equal(lg, c["logits"]) and torch.equal(off.nan_to_num(7.0), P.to16(c["offset"]).nan_to_num(7.0)) and torch.equal(pad, c["pad"])
    from jspsr_amd import ops                                        # the package's own view of the layout
    lg2, off2 = ops.split_head(h)
    assert torch.equal(lg2.permute(0, 3, 1, 2), lg) and torch.equal(off2.permute(0, 3, 1, 2).nan_to_num(7.0), off.nan_to_num(7.0))
