"""GPU parity of K1s (csrc/prop_steps.hip: one general propagation step, forward and backward with the raster gradient)
against tests/prop_steps_ref.py in fp64, element by element, and the guarantees of its fixed-point raster gradient.

Tolerance (`_atol`): the kernel and a plain fp32 evaluation share the dominant error, the fp32 sampling coordinate, so
the absolute tolerance of every quantity is taken from the REFERENCE, never from the kernel: 4 x max |fp32 - fp64| of
prop_steps_ref on the same inputs (the kernel orders its nine-term sums and contracts FMAs differently), floored at 4 ulp
of the largest |ref|, and asserted to stay under 5e-4 for unit-scale data.  On top of it 1e-5 * |ref| per element.
Observed fp32 floors (max |fp32 - fp64| over the parity matrix, CPU; the largest of each is at 3 x 45 x 200): out 6.8e-6,
grad_weight 1.2e-5, grad_offset 1.9e-5, grad_dem 5.1e-5, grad_wk 9.8e-5 (so the largest derived atol is 3.9e-4), grad_b0
2.1e-5; at the shapes of one tile or less all of them are under 7e-6.
The cap and the data: prop_steps_ref.case draws the raster with amplitude 0.5, not 1.  Five of the six quantities meet the
5e-4 cap at amplitude 1 as well (largest derived atol 2.0e-4, grad_dem, which does not depend on the raster); grad_wk -- a
sum over all B*H*W pixels, |grad_wk| ~ 50 at 3 x 45 x 200 -- does not (floor 2.0e-4, atol 7.8e-4): its floor is 27 000
coordinate roundings added up, each proportional to the raster's slope.  The amplitude was chosen for that one quantity;
error and signal halve together, so the relative sharpness of every check is what it would be at amplitude 1.
"""
import functools

import pytest
import torch

from tests import prop_steps_ref as PR

pytestmark = pytest.mark.gpu

RTOL = 1e-5
CAP = 5e-4                       # the derived atol may not exceed this for unit-scale data
EPS32 = 2.0 ** -23
TH, TW, HALO = 8, 64, 8          # K1s tile and halo (prop_steps.hip: STH, STW; prop_tile.h: HALO)
FEXP_MAX = 126                   # clamp of the per-tile fixed-point exponent (prop_steps.hip)
T_TILE = TH * TW * 9 + 1         # terms that can land in one window slot at most
T_SLOT = 37                      # nine taps x four corners + the residual term: what lands in a slot on average
QUANT = ("out", "grad_weight", "grad_offset", "grad_dem", "grad_wk", "grad_b0")
SEC2 = (2, 16, 128)

SHAPES = [
    (1, 1, 1),        # single pixel
    (2, 5, 3),        # tiny raster
    (1, 8, 64),       # exactly one 8 x 64 tile
    (2, 7, 63),       # one pixel short of a tile both ways
    (2, 9, 65),       # one pixel over a tile both ways
    (2, 16, 128),     # exact 2 x 2 tiles: every seam pixel has a neighbour window
    (1, 24, 130),     # W % 4 == 2
    (3, 45, 200),     # ragged both ways, 6 x 4 tiles
]


def _ops():
    from jspsr_amd import ops
    return ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _step_backward_full(gout, dem, weight, offset, wk, scale, normalize, accumulate, gweight, goffset, gdem, gwk, gb0, ws):
    """jspsr_prop_step_backward_f32 with grad_wk / grad_b0 (ops._step_backward always passes NULL for them)."""
    from jspsr_amd import _lib
    B, _, H, W = dem.shape
    lib = _lib.load()
    _lib.check(lib.jspsr_prop_step_backward_f32(gout.data_ptr(), dem.data_ptr(), weight.data_ptr(), offset.data_ptr(),
                                                offset.shape[1], wk.data_ptr(), float(scale), int(normalize), int(accumulate),
                                                gweight.data_ptr(), goffset.data_ptr(),
                                                gdem.data_ptr() if gdem is not None else None, gwk.data_ptr(), gb0.data_ptr(),
                                                ws.data_ptr(), B, H, W, _stream()), "jspsr_prop_step_backward_f32")


def _shifted(t):
    """A copy of `t` that starts one float into a larger device buffer: 4-byte aligned, not 16."""
    buf = torch.empty(t.numel() + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _prefill(c, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(c[s].shape, generator=g) for k, s in (("grad_weight", "weight"), ("grad_offset", "offset"), ("grad_dem", "dem"))}


def _run(c, scale, normalize, accumulate=0, pre=None, gout=None, full=True, shifted=False):
    """One forward and one backward of the kernels on the case `c` -> dict of CPU tensors.  Gradient buffers start from
    `pre` (accumulate) or NaN (overwritten; grad_dem, always added to, from zero).  full: through the C ABI with
    grad_wk / grad_b0; otherwise through ops._step_backward."""
    ops = _ops()
    dem, weight, offset, wk, b0 = (c[k].cuda() for k in ("dem", "weight", "offset", "wk", "b0"))
    gout = (c["gout"] if gout is None else gout).cuda()
    B, _, H, W = dem.shape
    out = torch.full_like(dem, float("nan"))
    if shifted:
        dem, out = _shifted(dem), _shifted(out)
    ops._step_forward(dem, weight, offset, wk, b0, scale, normalize, out)
    nan = float("nan")
    gw = pre["grad_weight"].cuda() if accumulate else torch.full_like(weight, nan)
    go = pre["grad_offset"].cuda() if accumulate else torch.full_like(offset, nan)
    gd = pre["grad_dem"].cuda() if pre is not None else torch.zeros_like(dem)
    if shifted:
        gd = _shifted(gd)
    ws = ops._step_workspace(B, H, W, "cuda")
    res = {}
    if full:
        gk, gb = torch.full((9,), nan, device="cuda"), torch.full((1,), nan, device="cuda")
        _step_backward_full(gout, dem, weight, offset, wk, scale, normalize, accumulate, gw, go, gd, gk, gb, ws)
        res.update(grad_wk=gk.cpu(), grad_b0=gb.cpu())
    else:
        ops._step_backward(gout, dem, weight, offset, wk, scale, normalize, accumulate, gw, go, gd, ws)
    torch.cuda.synchronize()
    res.update(out=out.cpu().clone(), grad_weight=gw.cpu(), grad_offset=go.cpu(), grad_dem=gd.cpu().clone())
    return res


@functools.lru_cache(maxsize=None)
def _case(shape, oc, seed=None):
    B, H, W = shape
    # (+ 1: with this stream no coordinate of the two tiny rasters sits on a kink, where one dropped tap is 0.4 % of the entries)
    return PR.case(B, H, W, oc, seed=1000 * B + 10 * H + W + oc + 1 if seed is None else seed)


def _refs(c, scale, normalize, gout=None):
    """(fp64, fp32) evaluations of prop_steps_ref on the case."""
    g = c["gout"] if gout is None else gout
    args = (c["dem"], c["weight"], c["offset"], c["wk"], c["b0"], scale, normalize, g)
    return PR.step_grads(*args, dtype=torch.float64), PR.step_grads(*args, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _matrix_refs(shape, oc, scale, normalize):
    return _refs(_case(shape, oc), scale, normalize)


def _atol(r64, r32, mask=None):
    """4 x the fp32 reference's own error, floored at 4 ulp of the largest |ref| -- and the floor itself."""
    d = (r32.double() - r64).abs()
    a = r64.abs()
    if mask is not None:
        d, a = d[mask], a[mask]
    floor = d.max().item() if d.numel() else 0.0
    big = a.max().item() if a.numel() else 0.0
    return max(4.0 * floor, 4.0 * EPS32 * big), floor


def _close(got, ref, atol, what, mask=None, rtol=RTOL):
    err = (got.double() - ref.double()).abs()
    tol = atol + rtol * ref.double().abs()
    bad = ~(err <= tol)                      # NaN in `got` is bad
    if mask is not None:
        bad = bad & mask
        err = torch.where(mask, err, torch.zeros_like(err))
    print(f"    {what}: max err {err.nan_to_num(float('inf')).max().item() if err.numel() else 0.0:.3e}  atol {atol:.3e}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, max err {err.nan_to_num(float('inf')).max().item():.3e}, atol {atol:.3e}"


def _compare_all(got, r64, r32, c, what, pre=None, accumulate=0, cap=CAP, keys=QUANT, drop_cap=0.002):
    B, _, H, W = c["dem"].shape
    smooth = PR.smooth_mask(c["offset"], H, W)
    dropped = 1.0 - smooth.sum().item() / PR.non_centre(c["offset"])
    print(f"  {what}: kink mask drops {dropped:.2e} of the non-centre offset entries")
    assert dropped <= drop_cap, f"{what}: the kink mask drops {dropped:.3e} of the offset gradient"
    for k in keys:
        if k not in got:
            continue
        mask = smooth if k == "grad_offset" else None
        atol, floor = _atol(r64[k], r32[k], mask)
        assert atol <= cap, f"{what} {k}: derived atol {atol:.3e} (fp32 floor {floor:.3e}) exceeds {cap:.1e}"
        ref = r64[k]
        if pre is not None and k == "grad_dem" or accumulate and k in ("grad_weight", "grad_offset"):
            ref = ref + pre[k].double()                 # the kernel adds into what the buffer holds
        _close(got[k].reshape(ref.shape), ref, atol, f"{what} {k} (fp32 floor {floor:.2e})", mask)


# ---- 1. forward and backward parity matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("oc", [18, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_matrix(shape, oc, normalize):
    """out, grad_weight, grad_offset, grad_dem, grad_wk, grad_b0 against fp64, element by element, for scale in {0, 0.7}
    and accumulate in {0, 1} (buffers pre-filled with known random values: result = prefill + gradient; grad_wk /
    grad_b0 are overwritten either way).  The NULL-grad_wk form that ops._step_backward calls gives the same bits."""
    c = _case(shape, oc)
    for scale in (0.0, 0.7):
        r64, r32 = _matrix_refs(shape, oc, scale, normalize)
        for accumulate in (0, 1):
            what = f"{shape} oc={oc} normalize={normalize} scale={scale} accumulate={accumulate}"
            pre = _prefill(c, 7) if accumulate else None
            got = _run(c, scale, normalize, accumulate, pre)
            _compare_all(got, r64, r32, c, what, pre, accumulate)
            assert torch.isfinite(got["grad_offset"]).all(), what           # the centre pair too: overwritten or added to
            via_ops = _run(c, scale, normalize, accumulate, pre, full=False)
            for k in ("out", "grad_weight", "grad_offset", "grad_dem"):
                assert torch.equal(got[k], via_ops[k]), f"{what} {k}: the NULL-grad_wk call differs"


@pytest.mark.parametrize("normalize,accumulate", [(0, 0), (1, 1)])
def test_pointers_aligned_to_4_bytes_only(normalize, accumulate):
    """dem, out and grad_dem one float into a larger buffer: W % 4 == 0 but no 16-byte loads of the DEM (dem_vec4 = 0, the
    case _SampleTaps makes whenever B*H*W is odd).  Same bits as the aligned run."""
    c = _case(SEC2, 16)
    pre = _prefill(c, 8) if accumulate else None
    a = _run(c, 0.7, normalize, accumulate, pre)
    b = _run(c, 0.7, normalize, accumulate, pre, shifted=True)
    for k in QUANT:
        assert torch.equal(a[k], b[k]), k
    _compare_all(b, *_refs(c, 0.7, normalize), c, "shifted", pre, accumulate)


# ---- 2. what the fixed-point accumulation guarantees ------------------------------------------------------------------
@pytest.mark.parametrize("normalize,accumulate,scale", [(0, 0, 0.7), (1, 0, 0.7), (0, 1, 0.7), (1, 1, 0.0)])
def test_bit_reproducible_without_far_taps(normalize, accumulate, scale):
    """No tap leaves tile + halo (|offset| <= 6.5 px): every output has the same bits in three runs."""
    c = _case(SEC2, 18)
    pre = _prefill(c, 9) if accumulate else None
    runs = [_run(c, scale, normalize, accumulate, pre) for _ in range(3)]
    for k in QUANT:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k
        assert torch.isfinite(runs[0][k]).all(), k


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("k", [-70, -40, -20, 20, 60])
def test_power_of_two_equivariance_is_exact(k, normalize):
    """grad_out * 2^k -> every gradient * 2^k, bit for bit: the per-tile scale absorbs the factor, the integers in LDS are
    the same ones.  (Breaks if the scale came from anything but the tile's own maximum, if a term were rounded before
    scaling, or if the write-back lost bits.)  |grad_out| * 2^k stays inside fp32's normal range and above 2^-81, down to
    which the scale follows the tile maximum: k = -70 (tile maximum about 2^-68) is past the earlier clamp of 100, which
    stopped at 2^-55."""
    c = _case(SEC2, 18)
    base = _run(c, 0.7, normalize)
    got = _run(c, 0.7, normalize, gout=c["gout"] * 2.0 ** k)
    for q in ("grad_dem", "grad_weight", "grad_offset", "grad_wk", "grad_b0"):
        exp = base[q] * 2.0 ** k
        assert torch.isfinite(exp).all() and (exp[base[q] != 0].abs() >= 2.0 ** -126).all(), q       # the claim needs normal numbers
        assert torch.equal(got[q], exp), f"{q}: {(got[q] != exp).sum().item()} elements differ"


@pytest.mark.parametrize("k", [-90, -110])
def test_beyond_the_exponent_clamp_the_error_is_bounded(k):
    """The per-tile exponent is clamped at 126 (2^126 is the largest power of two that leaves v * 2^fexp <= 2^46 finite in
    fp32 with room to spare), so the scale follows the tile maximum down to 2^-81.  Below that it saturates: one fixed-
    point unit is 2^-126 whatever the data, each term is rounded to a unit (off by half of one at most), and at most
    8*64*9 + 1 terms land in a slot -> |error| <= T * 2^-126 + the fp32 floor scaled by 2^k, at every pixel."""
    c = _case(SEC2, 18)
    r64, r32 = _refs(c, 0.7, 0)
    atol, _ = _atol(r64["grad_dem"], r32["grad_dem"])
    got = _run(c, 0.7, 0, gout=c["gout"] * 2.0 ** k, full=False)["grad_dem"].double()
    ref = r64["grad_dem"] * 2.0 ** k
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    bound = T_TILE * 2.0 ** -FEXP_MAX + (atol + RTOL * r64["grad_dem"].abs()) * 2.0 ** k
    print(f"    2^{k}: max err {err.max().item():.3e} = {err.max().item() * 2.0 ** FEXP_MAX:.1f} units, bound {bound.min().item():.3e}")
    assert bool((err <= bound).all()), f"max err {err.max().item():.3e}, bound {bound.min().item():.3e}"


def test_below_half_a_fixed_point_unit_everything_rounds_to_zero():
    """grad_out * 2^-140 (fp32 denormals): every term times 2^126 is below 2^-10 units -> grad_dem stays exactly as it was."""
    c = _case(SEC2, 18)
    tiny = c["gout"] * 2.0 ** -140
    assert (tiny != 0).any()
    got = _run(c, 0.7, 0, gout=tiny, full=False)
    assert (got["grad_dem"] == 0).all()
    assert torch.isfinite(got["grad_weight"]).all() and torch.isfinite(got["grad_offset"]).all()


def _outlier_gout(c, r):
    """One pixel of every tile times 2^r -> (gout, far) with far = pixels more than 16 px from every outlier."""
    B, _, H, W = c["dem"].shape
    gout = c["gout"].clone()
    far = torch.ones(H, W, dtype=torch.bool)
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    for y in range(3, H, TH):
        for x in range(21, W, TW):
            gout[:, 0, y, x] *= 2.0 ** r
            far &= ((ys - y).abs() > 16) | ((xs - x).abs() > 16)
    return gout, far.view(1, 1, H, W).expand(B, 1, H, W)


def _tile_max(c, gout, scale, normalize):
    """The largest |contribution| of any tile (what sets the fixed-point scale), fp64."""
    m = c["weight"].double()
    if normalize:
        m = m - m.mean(1, keepdim=True)
    t = (gout.double() * c["wk"].double().view(1, 9, 1, 1) * m).abs().max().item()
    return max(t, (scale * gout.double()).abs().max().item())


@pytest.mark.parametrize("r", [10, 20, 30])
def test_dynamic_range_inside_one_tile(r):
    """grad_out ~ N(0,1) except one pixel per tile, times 2^r.  The scale puts the tile's largest term at [2^45, 2^46), so
    one unit is at most (tile max) * 2^-45 and a pixel that collects ~37 rounded terms is off by less than T_slot units plus the fp32
    floor -- asserted at every pixel with the floor of THIS input (outlier-scaled), and at the pixels more than 16 px from
    every outlier with the floor of those pixels alone (unit scale), so the small gradients are held to the fixed-point
    bound and not merely to the outlier's tolerance.  What that leaves the O(1) gradients (|grad_dem| ~ 3, tile max
    ~ 2^(r+2)): the bound is 4e-9 at r = 10, 4e-6 at r = 20, 4e-3 at r = 30, i.e. about 30, 20 and 10 bits.  Terms are
    rounded to the nearest unit, not truncated: replaying the scatter's arithmetic on the CPU for this input at r = 30,
    truncation leaves the far pixels 0.73 units short along sign(ref) on average (mean |error| 1.4 units, max 10.5), rounding
    0.02 units (mean |error| 0.6, max 4.5).  So at r = 30 both the mean signed error and the mean error along sign(ref) of the
    far pixels must stay under a tenth of their mean absolute error."""
    c = _case(SEC2, 18)
    gout, far = _outlier_gout(c, r)
    r64, r32 = _refs(c, 0.7, 0, gout)
    got = _run(c, 0.7, 0, gout=gout, full=False)["grad_dem"].double()
    ref = r64["grad_dem"]
    unit = _tile_max(c, gout, 0.7, 0) * 2.0 ** -45
    err = got - ref
    atol_all, _ = _atol(ref, r32["grad_dem"])
    atol_far, floor_far = _atol(ref, r32["grad_dem"], far)
    assert atol_far <= CAP, atol_far
    e_far, ref_far = err[far], ref[far]
    shrink = (e_far * torch.sign(ref_far)).mean().item()
    print(f"    r={r}: unit {unit:.3e}; all pixels max err {err.abs().max().item():.3e} (atol {atol_all:.3e}); far pixels max err "
          f"{e_far.abs().max().item():.3e} = {e_far.abs().max().item() / unit:.2f} units (fp32 floor {floor_far:.2e}), mean signed "
          f"{e_far.mean().item():.3e}, mean abs {e_far.abs().mean().item():.3e}, mean err along sign(ref) {shrink:.3e}")
    assert bool((err.abs() <= T_SLOT * unit + atol_all + RTOL * ref.abs()).all())
    assert bool((e_far.abs() <= T_SLOT * unit + atol_far + RTOL * ref_far.abs()).all())
    if r == 30:
        assert abs(e_far.mean().item()) < 0.1 * e_far.abs().mean().item()
        assert abs(shrink) < 0.1 * e_far.abs().mean().item()


def test_zero_gradient_tile():
    """grad_out zero on one whole tile (its scale takes the t_ > 0 false branch), random elsewhere: the result is the
    neighbours' contribution alone, as in fp64; an image whose tiles are all zero receives exactly nothing."""
    c = _case(SEC2, 18)
    gout = c["gout"].clone()
    gout[0, :, :TH, TW:2 * TW] = 0
    r64, r32 = _refs(c, 0.7, 0, gout)
    got = _run(c, 0.7, 0, gout=gout)
    _compare_all(got, r64, r32, c, "zero tile")
    assert (got["grad_weight"][0, :, :TH, TW:2 * TW] == 0).all() and (got["grad_offset"][0, :, :TH, TW:2 * TW] == 0).all()
    gout[1] = 0
    pre = _prefill(c, 10)
    got = _run(c, 0.7, 0, pre=pre, gout=gout, full=False)
    assert torch.equal(got["grad_dem"][1], pre["grad_dem"][1])          # exactly nothing added
    assert (got["grad_weight"][1] == 0).all() and (got["grad_offset"][1] == 0).all()


def test_non_finite_grad_out():
    """One NaN and one +inf pixel in grad_out: their taps are dropped from grad_dem (finite everywhere, equal to the
    reference with those two entries set to 0), while grad_weight at the two pixels is non-finite -- the event is not lost,
    the optimizer's `bad` count sees it."""
    c = _case(SEC2, 18)
    spots = [(0, 2, 10), (1, 12, 100)]
    gout, clean = c["gout"].clone(), c["gout"].clone()
    for (b, y, x), v in zip(spots, (float("nan"), float("inf"))):
        gout[b, 0, y, x] = v
        clean[b, 0, y, x] = 0
    for normalize in (0, 1):
        r64, r32 = _refs(c, 0.7, normalize, clean)
        got = _run(c, 0.7, normalize, gout=gout, full=False)
        assert torch.isfinite(got["grad_dem"]).all()
        atol, _ = _atol(r64["grad_dem"], r32["grad_dem"])
        _close(got["grad_dem"], r64["grad_dem"], atol, f"grad_dem normalize={normalize}")
        ok = torch.ones_like(c["gout"], dtype=torch.bool)
        for b, y, x in spots:
            assert not torch.isfinite(got["grad_weight"][b, :, y, x]).any()
            ok[b, 0, y, x] = False
        atol, _ = _atol(r64["grad_weight"], r32["grad_weight"])
        _close(got["grad_weight"], r64["grad_weight"], atol, "grad_weight elsewhere", ok.expand_as(got["grad_weight"]))


# ---- 3. far taps and the raster border --------------------------------------------------------------------------------
def _place(off, b, k, y, x, py, px):
    """Tap k of pixel (b, y, x) samples at (py, px)."""
    off[b, 2 * k, y, x] = py - (y - 1 + k // 3)
    off[b, 2 * k + 1, y, x] = px - (x - 1 + k % 3)


# (b, tap, y, x, py, px): taps that land INSIDE the raster beyond their tile's window (only possible sideways at H = 16), at
# fractional positions, so all four corners carry weight: the global reads of the forward and all four float atomics
FAR_INSIDE = [(0, 1, 3, 5, 4.3, 100.6), (0, 0, 0, 20, 0.4, 90.7), (0, 8, 7, 63, 14.6, 126.2), (0, 5, 12, 40, 9.7, 75.3),
              (1, 2, 15, 0, 6.2, 110.9), (0, 3, 2, 100, 3.6, 30.3), (0, 6, 6, 64, 12.3, 0.4), (1, 7, 9, 127, 1.8, 54.6),
              (1, 0, 14, 90, 13.4, 10.7), (1, 8, 10, 70, 0.7, 47.2)]


def _fallback_taps(c):
    """The kernel's own rule (prop_tile.h corners_fast, prop_steps.hip scatter_corners) replayed on fp32 coordinates:
    (B,9,H,W) mask of the taps that leave tile + halo yet have all four corners inside the raster with non-zero weight."""
    off = PR.to18(c["offset"])
    B, _, H, W = off.shape
    f = torch.float32
    ys, xs = torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
    ky = torch.tensor([k // 3 - 1 for k in range(9)]).view(1, 9, 1, 1)
    kx = torch.tensor([k % 3 - 1 for k in range(9)]).view(1, 9, 1, 1)
    o = off.reshape(B, 9, 2, H, W)
    py, px = (ys + ky).to(f) + o[:, :, 0], (xs + kx).to(f) + o[:, :, 1]
    fy, fx = py.floor(), px.floor()
    inside = (fy >= 0) & (fy + 1 <= H - 1) & (fx >= 0) & (fx + 1 <= W - 1)          # False for NaN / inf
    ry = fy - ((ys // TH) * TH - HALO)
    rx = fx - ((xs // TW) * TW - HALO)
    inl = (ry >= 0) & (ry < TH + 2 * HALO - 1) & (rx >= 0) & (rx < TW + 2 * HALO - 1)
    return inside & ~inl & (py != fy) & (px != fx)


def _far_case():
    B, H, W = SEC2
    c = dict(PR.case(B, H, W, 18, seed=33))
    off = c["offset"].clone()
    off[0, :, :5, :9] *= 15.0                              # beyond tile + halo and beyond the raster
    off[0, 8:10] = 0
    inf, nan = float("inf"), float("nan")
    _place(off, 1, 0, 0, 40, -0.375, 40.25)                # py in (-1, 0)
    _place(off, 1, 2, 6, 126, 5.5, W - 0.25)               # px in (W - 1, W)
    _place(off, 1, 3, 9, 3, -1.0, 2.5)                     # exactly -1
    _place(off, 1, 5, 9, 120, 9.5, float(W))               # exactly W
    _place(off, 1, 6, 15, 64, H - 0.5, -0.75)              # both ends
    off[1, 0, 4, 70], off[1, 3, 4, 71] = inf, -inf
    off[1, 4, 4, 72], off[1, 7, 4, 73] = nan, 3.0e9
    off[0, 13, 12, 90], off[0, 12, 12, 90] = 3.0e9, nan
    for t in FAR_INSIDE:
        _place(off, *t)
    c["offset"] = off
    return c


@pytest.mark.parametrize("normalize", [0, 1])
def test_far_taps_and_the_border(normalize):
    """Taps beyond tile + halo (global fallback: plain global reads in the forward, float atomics in grad_dem) -- at least
    ten of them with all four corners inside the raster, counted with the kernel's own rule --, across the raster border,
    at exactly -1 / W, at +-inf, NaN and 3e9: everything element by element against fp64, finite.  (grad_dem's last bits
    depend on the order of the atomics here: no bit equality.)"""
    c = _far_case()
    fb = _fallback_taps(c)
    assert int(fb.sum()) >= len(FAR_INSIDE) and all(bool(fb[b, k, y, x]) for b, k, y, x, _, _ in FAR_INSIDE), int(fb.sum())
    r64, r32 = _refs(c, 0.7, normalize)
    got = _run(c, 0.7, normalize)
    for k in QUANT:
        assert torch.isfinite(got[k]).all(), k
    _compare_all(got, r64, r32, c, f"far taps normalize={normalize}")


def test_taps_outside_the_raster_contribute_exactly_nothing():
    """Pixels whose nine taps all have their four corners outside the raster (above, right of it, inside and outside the
    tile's window, +-inf, NaN, 3e9): out = b0 exactly, their grad_weight and grad_offset are exactly 0, and grad_dem has the
    bits of a run with grad_out zeroed at those pixels."""
    B, H, W = SEC2
    c = dict(_case(SEC2, 18))
    off = c["offset"].clone()
    inf, nan = float("inf"), float("nan")
    spots = [(0, 1, 5), (0, 9, 127), (1, 15, 64), (1, 7, 63)]
    where = [(-3.5, 20.5), (-1.25, 3.25), (4.5, float(W)), (H + 0.0, 7.5), (-40.5, -40.5), (3.0e9, 2.0), (inf, 1.0), (2.0, -inf), (nan, nan)]
    gout, clean = c["gout"].clone(), c["gout"].clone()
    for b, y, x in spots:
        for k, (py, px) in enumerate(where):
            _place(off, b, k, y, x, py, px)
        gout[b, 0, y, x] = clean[b, 0, y, x] * 2.0 ** -6     # (not the tile's largest term: the scale is the same in both runs)
        clean[b, 0, y, x] = 0
    c["offset"] = off
    got = _run(c, 0.0, 0, gout=gout, full=False)
    ref = _run(c, 0.0, 0, gout=clean, full=False)
    for b, y, x in spots:
        assert got["out"][b, 0, y, x].item() == c["b0"].item()
        assert (got["grad_weight"][b, :, y, x] == 0).all() and (got["grad_offset"][b, :, y, x] == 0).all()
    assert torch.isfinite(got["grad_dem"]).all() and torch.equal(got["grad_dem"], ref["grad_dem"])


# ---- 4. the two autograd shells ---------------------------------------------------------------------------------------
def _chain_case(fix):
    B, H, W = 2, 9, 65
    g = torch.Generator().manual_seed(51 + fix)
    feat = torch.randn(B, 1, H, W, generator=g)
    aff = torch.rand(B, 9, H, W, generator=g) / 4.5                     # sums to about 1: the chain neither dies nor blows up
    off = (2.0 * torch.randn(B, 18, H, W, generator=g)).clamp(-6.5, 6.5)
    off[:, 8:10] = 0
    ff = torch.rand(B, 1, H, W, generator=g)
    ff = torch.where(ff > 0.8, ff, torch.zeros_like(ff)) if fix else None
    probes = torch.randn(3, B, 1, H, W, generator=g)
    return feat, aff, off, ff, probes


def _chain_ref(feat, aff, off, ff, probes, lw, dtype):
    from oracle import nlspn_ref as NR
    leaves = [t.to(dtype).clone().requires_grad_() for t in (feat, aff, off)]
    fx = ff.to(dtype).clone().requires_grad_() if ff is not None else None
    steps = NR.propagate(leaves[0], leaves[2], leaves[1], 3, fx)
    loss = sum(w * (s * probes[i].to(dtype)).sum() for i, (w, s) in enumerate(zip(lw, steps)) if w)
    loss.backward()
    r = dict(steps=torch.cat([s.detach() for s in steps], 1), feat=leaves[0].grad, aff=leaves[1].grad, offset=leaves[2].grad)
    if fx is not None:
        r["feat_fix"] = fx.grad
    return r


@pytest.mark.parametrize("lw", [(1, 1, 1), (0, 0, 1), (1, 0, 0)], ids=["every-step", "last-step", "first-step"])
@pytest.mark.parametrize("fix", [0, 1], ids=["plain", "fix"])
def test_propagate_steps_chain(fix, lw):
    """ops.propagate_steps, 3 steps, against autograd in fp64 through oracle.nlspn_ref.propagate: the rasters, feat.grad,
    aff.grad, offset.grad (kink mask), feat_fix.grad -- with the loss on every step, on the last and on the first one only.
    (Autograd hands _PropagateSteps.backward zero tensors, not None, for the steps the loss does not use, so its
    `first` / `g is None` branches are not what differs between these cases: the overwrite-then-accumulate order over
    three steps and the flow of a gradient that enters at one end of the chain are.)"""
    ops = _ops()
    feat, aff, off, ff, probes = _chain_case(fix)
    r64 = _chain_ref(feat, aff, off, ff, probes, lw, torch.float64)
    r32 = _chain_ref(feat, aff, off, ff, probes, lw, torch.float32)
    d = [t.cuda().requires_grad_() for t in (feat, aff, off)]
    fx = ff.cuda().requires_grad_() if fix else None
    mask = ((ff > 0).sum(1, keepdim=True) > 0).float().cuda() if fix else None
    steps = ops.propagate_steps(d[0], d[1], d[2], 3, mask, fx)
    sum(w * (s * probes[i].cuda()).sum() for i, (w, s) in enumerate(zip(lw, steps)) if w).backward()
    got = dict(steps=torch.cat(steps, 1).detach().cpu(), feat=d[0].grad.cpu(), aff=d[1].grad.cpu(), offset=d[2].grad.cpu())
    if fix:
        got["feat_fix"] = fx.grad.cpu()
    B, _, H, W = feat.shape
    smooth = PR.smooth_mask(off, H, W)
    assert 1.0 - smooth.sum().item() / PR.non_centre(off) <= 0.002
    for k, ref in r64.items():
        m = smooth if k == "offset" else None
        atol, floor = _atol(ref, r32[k], m)
        assert atol <= CAP, (k, atol)
        _close(got[k], ref, atol, f"chain fix={fix} lw={lw} {k} (fp32 floor {floor:.2e})", m)


@pytest.mark.parametrize("legacy", [False, True])
def test_sample_taps_shell(legacy):
    """ops.sample_taps at B*H*W odd (seven of its eight output rasters are not 16-byte aligned) against
    oracle.nlspn_ref.sample_1x1: the eight sampled rasters and conf.grad."""
    from oracle import nlspn_ref as NR
    ops = _ops()
    B, H, W = 1, 7, 63
    g = torch.Generator().manual_seed(61)
    conf = torch.randn(B, 1, H, W, generator=g)
    off16 = (2.0 * torch.randn(B, 16, H, W, generator=g)).clamp(-6.5, 6.5)
    gout = torch.randn(B, 8, H, W, generator=g)

    def ref(dtype):
        cf = conf.to(dtype).clone().requires_grad_()
        taps = []
        for t in range(8):
            k = t if t < 4 else t + 1
            taps.append(NR.sample_1x1(cf, off16[:, 2 * t:2 * t + 2].to(dtype), (k // 3 - 1.0, k % 3 - 1.0) if legacy else (0.0, 0.0)))
        out = torch.cat(taps, 1)
        out.backward(gout.to(dtype))
        return dict(out=out.detach(), grad_conf=cf.grad)

    r64, r32 = ref(torch.float64), ref(torch.float32)
    cd = conf.cuda().requires_grad_()
    out = ops.sample_taps(cd, off16.cuda(), legacy)
    out.backward(gout.cuda())
    got = dict(out=out.detach().cpu(), grad_conf=cd.grad.cpu())
    for k in r64:
        atol, floor = _atol(r64[k], r32[k])
        assert atol <= CAP, (k, atol)
        _close(got[k], r64[k], atol, f"sample_taps legacy={legacy} {k} (fp32 floor {floor:.2e})")
