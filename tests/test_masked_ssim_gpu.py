"""GPU: SSIM over a validity plane under the "window" rule (K23: jspsr_loss_menu_valid_ssim_*, jspsr_ssim_tiles_forward)
through get_loss / get_criterion(ssim_valid="window"), metrics.ssim_tiles, PerformanceMeter(masked=True,
ssim_valid="window") and evaluate, against the restatement tests/masked_ssim_ref.py.

SSIM's tolerances follow tests/test_loss_menu_gpu.py::_tolerances: the value within 4 |v32 - v64| + 1e-6 and the gradient
within 4 max|g32 - g64| + 1e-4 max|g64|, v32 / g32 being the fp32 torch restatement of the same masked call.  The other keys
keep their K19 bounds (tests/test_masked_loss_gpu.py): 2e-6 max(1, |ref|) for L1 / L2 / Grad, 1e-5 |ref| + 1e-7 for BerHu;
the five-key criterion's gradient is the weighted sum of the families' gradients, so it is held to the sum of their bounds,
SSIM's taken at its own weight."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import batches_ref as BR
from tests import masked_ssim_ref as S

SHAPES = S.SHAPES
FIVE = {"L1": 1, "L2": 1, "Grad": 0.1, "SSIM": 0.5, "Berhu": 0.2}
K19 = {"L1": 1, "L2": 1, "Grad": 0.1, "Berhu": 0.2}
BASE = ("l1", "l2", "grad")
JUNK = (float("nan"), float("inf"), float("-inf"), -32767.0, 1e30)
LOSS_KERNELS = ("loss_valid_forward", "loss_valid_finalize", "loss_valid_backward", "loss_menu_valid_max", "loss_menu_valid_sum",
                "loss_menu_valid_combine", "loss_menu_valid_backward", "ssim_valid_forward", "ssim_valid_backward", "ssim_forward",
                "ssim_backward", "loss_menu_combine", "loss_forward")
METER_KERNELS = ("scores_batch_valid (lds)", "scores_batch_valid (stream)", "ssim_tiles_forward", "ssim_tiles_finalize", "ssim_forward",
                 "ssim_finalize")
# counted map elements per sample, valid mode, as the rule gives them on the CPU (tests/test_masked_ssim_cpu.py)
EXPECTED = {((2, 1, 23, 37), "pixel"): 2 * 230, ((2, 1, 23, 37), "corner"): 2 * 350, ((2, 1, 23, 37), "rect"): 2 * 327,
            ((2, 1, 23, 37), "island"): 1, ((2, 1, 23, 37), "sample"): 345, ((1, 2, 45, 76), "pixel"): 2 * 2189,
            ((1, 2, 45, 76), "rect"): 2 * 2264, ((1, 1, 11, 11), "ones"): 1, ((1, 1, 11, 11), "island"): 1}


def census(names):
    from jspsr_amd import _lib
    lib = _lib.load()
    return {k: lib.jspsr_launch_count(k.encode()) for k in names}


def dev(v, dtype=torch.bool):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda().to(dtype)


def run(crit, p, g, v, up=1.0):
    """-> ({key: 0-d device tensor}, gradient) of a Criterion / LossTerm call on the GPU."""
    x = p.cuda().requires_grad_()
    out = crit(x, g.cuda(), valid=v) if v is not None else crit(x, g.cuda())
    if not isinstance(out, dict):
        out = {"Total": out}
    (up * out["Total"]).backward()
    return {k: t.detach().clone() for k, t in out.items()}, x.grad.clone()


_REF = {}


def ref(shape, name, weights, up):
    """The fp64 restatement of one masked call and, for SSIM alone, the fp32 one (else None), made once and never changed."""
    key = (shape, name, tuple(weights.items()), up)
    if key not in _REF:
        p, g = S.pair(shape)
        v = S.planes(shape)[name]
        alone = all(k.lower() == "ssim" for k in weights)
        _REF[key] = (S.values_and_grad(weights, p, g, v, up=up),
                     S.values_and_grad(weights, p, g, v, up=up, dtype=torch.float32) if alone else None)
    return _REF[key]


def ssim_bounds(shape, name, up):
    """-> (v64, g64, N_s, value bound, gradient bound) of SSIM alone at scale `up`."""
    (v64, g64, n), (v32, g32, _) = ref(shape, name, {"ssim": 1.0}, up)
    dv = abs(v32["ssim"] - v64["ssim"])
    dg = (g32.double() - g64).abs().max().item()
    return v64["ssim"], g64, n, 4 * dv + 1e-6, 4 * dg + 1e-4 * g64.abs().max().item()


def gpu_count(p, g, v):
    """N_s as the device counts it: the per-tile form on the planes of the call (the same forward kernel instance)."""
    from jspsr_amd import metrics as M
    B, C, H, W = p.shape
    full = np.broadcast_to(v, p.shape).copy().reshape(B * C, 1, H, W)
    _, cnt = M.ssim_tiles(p.reshape(B * C, 1, H, W).cuda(), g.reshape(B * C, 1, H, W).cuda(), "piq", 0.0, valid=dev(full))
    return int(cnt.sum().item())


# ---- values and gradients ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_ssim_and_the_five_key_criterion_match_the_restatement(shape):
    from jspsr_amd.losses import get_criterion, get_loss
    p, g = S.pair(shape)
    for name, v in S.planes(shape).items():
        v64, g64, n, tv, tg = ssim_bounds(shape, name, 3.0)
        if (shape, name) in EXPECTED:
            assert n == EXPECTED[shape, name], (shape, name, n)
        if name == "speckle" and shape == (1, 2, 45, 76):
            assert 600 < n < 2 * 2310, n
        assert gpu_count(p, g, v) == n, (shape, name)
        out, gr = run(get_loss("ssim", ssim_valid="window"), p, g, dev(v), up=3.0)
        err = (gr.cpu().double() - g64).abs().max().item()
        print(shape, name, "N_s", n, "ssim", out["Total"].item(), v64, "bound", tv, "grad err", err, "bound", tg)
        assert abs(out["Total"].item() - v64) <= tv, (shape, name, out["Total"].item(), v64, tv)
        assert err <= tg, (shape, name, err, tg)
        # the five keys: SSIM enters the gradient with weight 0.5 at up = 2
        (r64, rg, _), _ = ref(shape, name, FIVE, 2.0)
        _, _, _, sv, sg = ssim_bounds(shape, name, 1.0)
        out, gr = run(get_criterion(FIVE, ssim_valid="window"), p, g, dev(v, torch.uint8), up=2.0)
        assert list(out) == list(FIVE) + ["Total"]
        for k in FIVE:
            tol = 2e-6 * max(1.0, abs(r64[k])) if k.lower() in BASE else (sv if k == "SSIM" else 1e-5 * abs(r64[k]) + 1e-7)
            assert abs(out[k].item() - r64[k]) <= tol, (shape, name, k, out[k].item(), r64[k], tol)
        total = sum(w * out[k].double().item() for k, w in FIVE.items())
        assert out["Total"].item() == np.float32(total), (shape, name)                  # in double, rounded once
        scale = rg.abs().max().item()
        err = (gr.cpu().double() - rg).abs().max().item()
        bound = 1e-6 * scale + 1e-9 + 1e-5 * scale + 1e-12 + sg
        print(shape, name, "five-key grad err", err, "bound", bound)
        assert err <= bound, (shape, name, err, bound)


@pytest.mark.parametrize("shape", SHAPES)
def test_all_ones_plane_has_the_bits_of_the_unmasked_call(shape):
    from jspsr_amd.losses import get_criterion, get_loss
    p, g = S.pair(shape)
    B, C, H, W = shape
    for crit in (get_loss("ssim", ssim_valid="window"), get_criterion(FIVE, ssim_valid="window")):
        want, wg = run(crit, p, g, None, up=1.5)
        for ones in (torch.ones((B, 1, H, W), dtype=torch.bool, device="cuda"), torch.full(shape, 255, dtype=torch.uint8, device="cuda")):
            got, gg = run(crit, p, g, ones, up=1.5)
            assert list(got) == list(want)
            assert all(torch.equal(got[k], want[k]) for k in want), (shape, str(crit), {k: (got[k].item(), want[k].item()) for k in want})
            assert torch.equal(gg.view(torch.int32), wg.view(torch.int32)), (shape, str(crit), (gg - wg).abs().max().item())


@pytest.mark.parametrize("shape", SHAPES)
def test_what_the_rasters_hold_at_masked_pixels_has_no_influence(shape):
    from jspsr_amd.losses import get_criterion, get_loss
    p, g = S.pair(shape)
    for name, v in S.planes(shape).items():
        if name == "ones":
            continue
        inv = torch.from_numpy(~np.broadcast_to(v, shape))
        for crit in (get_loss("ssim", ssim_valid="window"), get_criterion(FIVE, ssim_valid="window")):
            want, wg = run(crit, p, g, dev(v))
            assert all(torch.isfinite(t).all() for t in want.values()) and torch.isfinite(wg).all(), (shape, name)
            assert not wg.cpu().view(torch.int32)[inv].any(), (shape, name)          # +0.0 there: all 32 bits clear
            for i, junk in enumerate(JUNK):
                for where in ("pred", "gt", "both"):
                    p2, g2 = p.clone(), g.clone()
                    if where != "gt":
                        p2[inv] = junk
                    if where != "pred":
                        g2[inv] = JUNK[(i + 1) % len(JUNK)]
                    got, gg = run(crit, p2, g2, dev(v, torch.uint8) * 7)             # any non-zero byte is valid
                    assert all(torch.equal(got[k], want[k]) for k in want), (shape, name, junk, where)
                    assert torch.equal(gg.cpu().view(torch.int32), wg.cpu().view(torch.int32)), (shape, name, junk, where)


@pytest.mark.parametrize("shape", SHAPES)
def test_nothing_counted_gives_zero_not_nan(shape):
    from jspsr_amd.losses import get_criterion, get_loss
    p, g = S.pair(shape)
    p, g = p.clone(), g.clone()
    p[0, 0, 0, 0], g[0, 0, 1, 1] = float("nan"), -32767.0
    none = torch.zeros(shape, dtype=torch.bool, device="cuda")
    for crit in (get_loss("ssim", ssim_valid="window"), get_criterion(FIVE, ssim_valid="window"), get_criterion({"SSIM": 2.0, "L2": 1.0}, ssim_valid="window")):
        out, gr = run(crit, p, g, none)
        assert all(t.item() == 0.0 for t in out.values()), (shape, str(crit), out)
        assert not gr.cpu().view(torch.int32).any(), (shape, str(crit))
    # pixels are valid but no window is whole: SSIM 0 with gradient 0, the other keys finite and at work
    if shape[2] > 11:
        grid = torch.ones(shape, dtype=torch.bool)
        grid[..., ::6, ::6] = False
        q, h = S.pair(shape)
        out, gr = run(get_criterion(FIVE, ssim_valid="window"), q, h, grid.cuda())
        assert out["SSIM"].item() == 0.0 and out["L1"].item() > 0 and all(torch.isfinite(t) for t in out.values())
        assert torch.isfinite(gr).all() and gr.any()
        out, gr = run(get_loss("ssim", ssim_valid="window"), q, h, grid.cuda())
        assert out["Total"].item() == 0.0 and not gr.cpu().view(torch.int32).any()


def test_a_nan_at_a_valid_pixel_of_gt_poisons_as_in_the_unmasked_call():
    from jspsr_amd.losses import get_loss
    shape = (2, 1, 23, 37)
    p, g = S.pair(shape)
    g = g.clone()
    g[1, 0, 5, 5] = float("nan")
    crit = get_loss("ssim", ssim_valid="window")
    plain, _ = run(crit, p, g, None)
    masked, _ = run(crit, p, g, dev(S.planes(shape)["corner"]))
    assert torch.isnan(plain["Total"]) and torch.isnan(masked["Total"])
    v = S.planes(shape)["corner"].copy()
    v[1, 0, 5, 5] = False                                                            # masked out: no influence
    out, gr = run(crit, p, g, dev(v))
    assert torch.isfinite(out["Total"]) and torch.isfinite(gr).all()


def test_rectangle_plane_is_the_unmasked_call_on_the_cropped_tensors():
    """Valid mode: the counted windows are exactly those inside the rectangle.  (It does not hold in same mode, where the
    crop's padding is not void: tests/test_masked_ssim_cpu.py.)  Both sides are fp32 sums of the same terms in another
    order, so their difference is held to the bound either has against fp64."""
    from jspsr_amd.losses import get_loss
    from tests import loss_menu_ref as M
    crit = get_loss("ssim", ssim_valid="window")
    for shape, (y0, y1, x0, x1) in (((2, 1, 23, 37), (3, 19, 5, 30)), ((1, 2, 45, 76), (0, 45, 20, 70)), ((3, 1, 43, 54), (16, 27, 11, 54))):
        p, g = S.pair(shape)
        v = np.zeros((shape[0], 1) + shape[2:], bool)
        v[..., y0:y1, x0:x1] = True
        pc, gc = p[..., y0:y1, x0:x1].contiguous(), g[..., y0:y1, x0:x1].contiguous()
        v64, g64 = M.value_and_grad(M.ssim_loss, pc, gc)
        x = pc.clone().requires_grad_()
        v32 = M.ssim_loss(x, gc)
        v32.backward()
        tv = 4 * abs(v32.item() - v64) + 1e-6
        tg = 4 * (x.grad.double() - g64).abs().max().item() + 1e-4 * g64.abs().max().item()
        got, gg = run(crit, p, g, dev(v))
        want, wg = run(crit, pc, gc, None)
        assert gpu_count(p, g, v) == shape[0] * shape[1] * (y1 - y0 - 10) * (x1 - x0 - 10)
        print(shape, got["Total"].item(), want["Total"].item(), v64, tv)
        assert abs(got["Total"].item() - want["Total"].item()) <= tv and abs(got["Total"].item() - v64) <= tv
        assert (gg[..., y0:y1, x0:x1] - wg).abs().max().item() <= tg
        outside = torch.from_numpy(~np.broadcast_to(v, shape))
        assert not gg.cpu().view(torch.int32)[outside].any()


def test_masked_criterion_with_ssim_captures_in_a_graph():
    """Forward + backward captured on one stream; a replay after the plane's contents (and pred) change in place equals the
    eager result bit for bit: N, N_g, N_s and BerHu's threshold are recomputed on the device."""
    from jspsr_amd.losses import get_criterion
    crit = get_criterion(FIVE, ssim_valid="window")
    shape = (2, 1, 64, 80)
    p0, g0 = S.pair(shape)
    p1 = S.pair(shape, seed=7)[0] * 1.1 - 0.02
    rs = np.random.RandomState(5)
    v0, v1 = rs.rand(2, 1, 64, 80) >= 0.002, rs.rand(2, 1, 64, 80) >= 0.004
    v1[1] = False
    g = g0.cuda()
    x = p0.cuda().requires_grad_()
    plane = dev(v0, torch.uint8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                               # warm up off the capture
            x.grad = None
            crit(x, g, valid=plane)["Total"].backward()
    torch.cuda.current_stream().wait_stream(s)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crit(x, g, valid=plane)
        out["Total"].backward()
    with torch.no_grad():
        x.copy_(p1.cuda())
        plane.copy_(dev(v1, torch.uint8))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: t.clone() for k, t in out.items()}
    got_g = x.grad.clone()
    want, want_g = run(crit, p1, g0, dev(v1, torch.uint8))
    assert all(torch.equal(got[k].detach(), want[k]) for k in want), {k: (got[k].item(), want[k].item()) for k in want}
    assert torch.equal(got_g, want_g)
    assert not got_g[1].any() and got_g[0].any() and 0 < want["SSIM"].item() < 1


def test_refusals_before_any_launch():
    from jspsr_amd.losses import get_criterion, get_loss
    x = torch.rand(2, 1, 16, 20, device="cuda")
    ok = torch.ones(2, 1, 16, 20, dtype=torch.bool, device="cuda")
    c0 = census(LOSS_KERNELS)
    for crit in (get_loss("ssim"), get_criterion({"L1": 1, "SSIM": 0.5})):           # the default still refuses
        with pytest.raises(NotImplementedError, match="SSIM"):
            crit(x, x, valid=ok)
    crit = get_criterion(FIVE, ssim_valid="window")
    for bad in (ok[:1], ok[:, :, :15], ok.expand(2, 3, 16, 20)):
        with pytest.raises(ValueError, match="valid"):
            crit(x, x, valid=bad)
    with pytest.raises(TypeError, match="valid"):
        crit(x, x, valid=ok.float())
    with pytest.raises(ValueError, match="H, W >= 11"):
        crit(x[..., :10, :], x[..., :10, :], valid=ok[..., :10, :])
    assert census(LOSS_KERNELS) == c0


def test_launch_census_of_the_criterion():
    """The masked criterion with SSIM = the K19 masked pair + one forward and one backward launch."""
    from jspsr_amd.losses import get_criterion
    shape = (2, 1, 23, 37)
    p, g = S.pair(shape)
    v = dev(S.planes(shape)["rect"])
    c0 = census(LOSS_KERNELS)
    run(get_criterion(K19), p, g, v)
    c1 = census(LOSS_KERNELS)
    run(get_criterion(FIVE, ssim_valid="window"), p, g, v)
    c2 = census(LOSS_KERNELS)
    k19 = {k: c1[k] - c0[k] for k in LOSS_KERNELS}
    ours = {k: c2[k] - c1[k] for k in LOSS_KERNELS}
    assert k19["ssim_valid_forward"] == 0 and k19["ssim_valid_backward"] == 0 and sum(k19.values()) == 7
    assert ours == dict(k19, ssim_valid_forward=1, ssim_valid_backward=1), (k19, ours)
    # without a plane the keyword changes nothing: the unmasked kernels
    run(get_criterion(FIVE, ssim_valid="window"), p, g, None)
    c3 = census(LOSS_KERNELS)
    assert c3["ssim_valid_forward"] == c2["ssim_valid_forward"] and c3["ssim_forward"] == c2["ssim_forward"] + 1


# ---- the per-tile form -------------------------------------------------------------------------------------------------
def tile_batch():
    """Five 64 x 64 tiles and a plane: sparse dropouts, a void tile in the middle, a lake at a border, an all-valid tile."""
    p, g = S.pair((5, 1, 64, 64), seed=61)
    rs = np.random.RandomState(62)
    v = rs.rand(5, 1, 64, 64) >= 0.003
    v[2] = False
    v[3] = True
    v[3, 0, 5:30, 44:] = False
    v[4] = True
    return p, g, v


@pytest.mark.parametrize("package", ["piq", "local"])
def test_ssim_tiles_against_the_restatement(package):
    from jspsr_amd import metrics as M
    p, g, v = tile_batch()
    w = M.local_window()
    want, wc = S.tiles(p, g, v, package, 0.05, window=w)
    w32, _ = S.tiles(p, g, v, package, 0.05, window=w, dtype=torch.float32)
    inv = torch.from_numpy(~v)
    p2, g2 = p.clone(), g.clone()
    p2[inv], g2[inv] = float("nan"), 1e30
    got, cnt = M.ssim_tiles(p2.cuda(), g2.cuda(), package, 0.05, valid=dev(v))
    assert got.shape == (5,) and got.dtype == torch.float32 and cnt.shape == (5,) and cnt.dtype == torch.int32
    assert cnt.cpu().tolist() == wc.tolist(), (cnt, wc)
    full = 48 * 48 if package == "piq" else 58 * 58
    assert wc[2] == 0 and wc[4] == full and 0 < wc[0] < full and 0 < wc[1] < full and 0 < wc[3] < full
    got = got.cpu().double().numpy()
    assert np.isnan(got[2]) and np.isnan(want[2])
    for b in (0, 1, 3, 4):
        tol = 4 * abs(w32[b] - want[b]) + 1e-6
        print(package, b, int(wc[b]), got[b], want[b], tol)
        assert abs(got[b] - want[b]) <= tol, (package, b, got[b], want[b], tol)
    # the void tile does not change its neighbours' bits; nor do their batch mates' planes
    keep = [0, 1, 3, 4]
    rest, rc = M.ssim_tiles(p2[keep].cuda(), g2[keep].cuda(), package, 0.05, valid=dev(v[keep]))
    first, fc = M.ssim_tiles(p[:1].cuda(), g[:1].cuda(), package, 0.05, valid=dev(v[:1], torch.uint8) * 9)
    whole, _ = M.ssim_tiles(p2.cuda(), g2.cuda(), package, 0.05, valid=dev(v))
    assert torch.equal(rest.view(torch.int32), whole[keep].view(torch.int32)) and rc.cpu().tolist() == wc[keep].tolist()
    assert torch.equal(first.view(torch.int32), whole[:1].view(torch.int32)) and fc.item() == wc[0]


@pytest.mark.parametrize("package", ["piq", "local"])
@pytest.mark.parametrize("size,border", [((64, 64), 0.05), ((23, 37), 0.0), ((45, 76), 0.1)])
def test_ssim_tiles_without_a_plane_and_with_all_ones_has_the_bits_of_ssim(package, size, border):
    from jspsr_amd import metrics as M
    B = 3
    p, g = S.pair((B, 1) + size, seed=63)
    pc, gc = p.cuda(), g.cuda()
    H, W = size
    h, w = H - 2 * int(H * border), W - 2 * int(W * border)
    want = torch.stack([M.ssim(*M.prepare(pc[b:b + 1], gc[b:b + 1], border), package) for b in range(B)])
    plain = M.ssim_tiles(pc, gc, package, border)
    assert torch.is_tensor(plain) and plain.shape == (B,)
    ones, cnt = M.ssim_tiles(pc, gc, package, border, valid=torch.ones_like(pc, dtype=torch.bool))
    assert torch.equal(plain.view(torch.int32), want.view(torch.int32)), (plain, want)
    assert torch.equal(ones.view(torch.int32), want.view(torch.int32)), (ones, want)
    assert cnt.cpu().tolist() == [(h - 10) * (w - 10) if package == "piq" else h * w] * B


def test_ssim_tiles_refusals():
    from jspsr_amd import metrics as M
    x = torch.rand(2, 1, 32, 32, device="cuda")
    ok = torch.ones_like(x, dtype=torch.bool)
    c0 = census(METER_KERNELS)
    for bad in (ok[:1], ok.float(), ok.cpu(), ok[:, 0]):
        with pytest.raises(ValueError, match="valid"):
            M.ssim_tiles(x, x, "piq", 0.0, valid=bad)
    with pytest.raises(ValueError):
        M.ssim_tiles(x, x, "piq", 0.5)
    with pytest.raises(ValueError, match=">= 11"):
        M.ssim_tiles(x[..., :12, :], x[..., :12, :], "piq", 0.1)
    with pytest.raises(NotImplementedError):
        M.ssim_tiles(x, x, "skimage")
    with pytest.raises(ValueError):
        M.ssim_tiles(x.expand(2, 2, 32, 32), x.expand(2, 2, 32, 32))
    assert census(METER_KERNELS) == c0


# ---- the meter and evaluate ------------------------------------------------------------------------------------------------
ELEV = (BR.PARAMS["elev_min"], BR.PARAMS["elev_max"], BR.PARAMS["elev_log"])


def masked_meter(metrics=None):
    from jspsr_amd import evaluate as EV
    cfg = metrics or {"RMSE": {"package": "local"}, "SSIM": {"package": "piq"}, "ssim": {"package": "local"}}
    return EV.PerformanceMeter(cfg, ELEV[0], ELEV[1], border=0.05, elev_log=ELEV[2], masked=True, ssim_valid="window")


def test_meter_update_launches_the_same_for_one_tile_and_five():
    from jspsr_amd import metrics as M
    p, g, v = tile_batch()
    pc, gc, vc = p.cuda(), g.cuda(), dev(v)
    per = {}
    for B in (1, 5):
        m = masked_meter()
        c0 = census(METER_KERNELS)
        m.update(pc[:B], gc[:B], valid=vc[:B])
        c1 = census(METER_KERNELS)
        per[B] = {k: c1[k] - c0[k] for k in METER_KERNELS}
    assert per[1] == per[5], per
    assert per[5]["ssim_tiles_forward"] == 2 and per[5]["ssim_tiles_finalize"] == 2 and per[5]["ssim_forward"] == 0      # one call per SSIM entry
    assert sum(per[5].values()) == 5
    # the columns are ssim_tiles' and the counts ride beside K20's
    m = masked_meter()
    m.update(pc, gc, valid=vc)
    table, cnt = m.table()[0], m.counts()
    assert m.count_names == list(M.COUNT_COLUMNS) + ["N_SSIM", "N_ssim"] and cnt.shape == (5, 5) and table.shape == (5, 3)
    for j, package in ((1, "piq"), (2, "local")):
        vals, c = M.ssim_tiles(pc, gc, package, 0.05, valid=vc)
        assert table[:, j].tobytes() == vals.cpu().numpy().tobytes() and cnt[:, 2 + j].tolist() == c.cpu().tolist()
    assert np.isnan(table[2]).all() and cnt[2].tolist() == [0] * 5
    score = m.get_score()
    for j, k in enumerate(("RMSE", "SSIM", "ssim")):
        assert score[k] == sum(float(x) for x in table[[0, 1, 3, 4], j]) / 4


class Stub(torch.nn.Module):
    """A model that needs no weights: the low-resolution DEM, bent a little."""

    def forward(self, *inputs):
        return inputs[0][:, 0:1] * 0.96 + 0.015


IC = {"lr_dem": 1, "image": 3, "mask": 15}


@pytest.fixture(scope="module")
def scenes():
    from jspsr_amd import data as D
    raw = BR.make_scenes([(100, 100), (96, 96)], seed=71)
    rs = np.random.RandomState(72)
    for i, s in enumerate(raw):
        hr = s["hr_dem"].copy()
        h, w = hr.shape[:2]
        hr[5:30, w - 20:] = -32767.0                       # a lake that touches the border
        hr[60 + i:66, 10:23] = np.nan                      # a cloud
        hr[rs.rand(h, w) < 0.002] = -32767.0               # a few sensor dropouts: 11 x 11 windows survive
        s["hr_dem"] = hr
    kinds = {k: [s[k] for s in raw] for k in ("lr_dem", "hr_dem", "image", "mask")}
    return D.DeviceScenes(**kinds, device="cuda:0", hr_nodata=-32767, **BR.PARAMS)


def test_evaluate_on_a_store_with_voids_equals_the_loop_over_tiles(scenes, monkeypatch):
    from jspsr_amd import data as D
    from jspsr_amd import evaluate as EV
    from jspsr_amd import losses as L
    from jspsr_amd import metrics as M
    cfg = {"L1": 1.0, "SSIM": 0.5, "Grad": 0.1}
    model = Stub().cuda()
    runs = {}
    for bs in (3, 1):
        meter = masked_meter()
        res = EV.evaluate(model, D.TileCropBatches(scenes, bs, 64, 4), L.get_criterion(cfg, ssim_valid="window"), meter, "JSPSR", IC)
        runs[bs] = (res, meter.table()[0], meter.counts())
    crit = L.get_criterion(cfg, ssim_valid="window")
    rows, counts, losses = [], [], []
    with torch.no_grad():
        for batch in D.TileCropBatches(scenes, 1, 64, 4):
            inputs, gt, _, _ = D.batch_pair(batch, "JSPSR", IC)
            pred = model(*inputs)
            s, c = M.batch_scores(pred, gt, ELEV[0], ELEV[1], 0.05, ELEV[2], valid=batch["valid"])
            sp, cp = M.ssim_tiles(pred, gt, "piq", 0.05, valid=batch["valid"])
            sl, cl = M.ssim_tiles(pred, gt, "local", 0.05, valid=batch["valid"])
            rows.append(torch.stack((s[:, 2], sp, sl), dim=1).cpu().numpy())
            counts.append(torch.cat((c, cp.reshape(-1, 1), cl.reshape(-1, 1)), dim=1).cpu().numpy())
            crit.reset()
            out = crit(pred, gt, valid=batch["valid"])
            losses.append({k: float(t.item()) for k, t in out.items()})
    rows, counts = np.concatenate(rows), np.concatenate(counts)
    assert len(rows) == 8 and (counts[:, 0] < 58 * 58).any() and (counts[:, 3] > 0).any() and (counts[:, 3] < 48 * 48).any()
    for bs in (1, 3):                     # the stub is elementwise: a tile's prediction does not depend on its batch
        res, table, cnt = runs[bs]
        assert np.array_equal(cnt, counts) and table.tobytes() == rows.tobytes(), bs
        want = {}
        for j, name in enumerate(("RMSE", "SSIM", "ssim")):
            keep = counts[:, (0, 3, 4)[j]] > 0
            want[name] = sum(float(x) for x in rows[keep, j]) / int(keep.sum())
        assert res[0] == want and all(np.isfinite(x) for x in want.values())
        for k in cfg:
            mean = sum(d[k] for d in losses) / len(losses)
            assert abs(res[2][k] - mean) <= 1e-12 * abs(mean), (bs, k, res[2][k], mean)
        mean = sum(d["Total"] for d in losses) / len(losses)
        assert abs(res[1] - mean) <= 1e-12 * abs(mean)
    # one device-to-host copy per pass, counted
    calls = {"n": 0}

    def counted(fn):
        def wrapper(*a, **k):
            calls["n"] += 1
            return fn(*a, **k)
        return wrapper

    batches = D.TileCropBatches(scenes, 3, 64, 4)
    list(batches)                                                    # the tile table is uploaded before the count starts
    meter = masked_meter()
    monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "item", counted(torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "cpu", counted(torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "tolist", counted(torch.Tensor.tolist))
    res = EV.evaluate(model, batches, crit, meter, "JSPSR", IC)
    meter.table()
    meter.counts()
    meter.worst("SSIM")
    monkeypatch.undo()
    assert calls["n"] == 1, calls
    assert res[0] == runs[3][0][0]
