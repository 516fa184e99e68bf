"""GPU: the masked losses (K19: jspsr_loss_valid_*, jspsr_loss_menu_valid_*) through MultiLoss / get_loss / get_criterion with
`valid=`, against the fp64 restatement tests/masked_loss_ref.py.

Tolerances are the unmasked tests' own: the base terms 2e-6 max(1, |ref|) on values and 1e-6 max|grad| + 1e-9 on gradients
(test_train_step_gpu.py), BerHu / BCE / Norm 1e-5 |v| + 1e-7 and 1e-5 scale + 1e-12 (test_loss_menu_gpu.py).  The five-key
criterion's gradient is the weighted sum of both families' gradients, so it is held to the sum of the two bounds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import masked_loss_ref as V

SHAPES = [(1, 1, 5, 3), (2, 1, 37, 53), (3, 2, 19, 70)]
FIVE = {"L1": 1, "L2": 1, "Grad": 0.1, "Berhu": 0.2, "BCE": 0.5}
BASE = ("l1", "l2", "grad", "edge", "mse")
KERNELS = ("loss_valid_forward", "loss_valid_finalize", "loss_valid_backward", "loss_menu_valid_max", "loss_menu_valid_sum",
           "loss_menu_valid_combine", "loss_menu_valid_backward", "loss_forward", "loss_menu_sum")
JUNK = (float("nan"), float("inf"), float("-inf"), -32767.0)


def planes(shape, seed=0):
    """name -> bool plane, (B,1,H,W) except "random" of a C > 1 shape, which is per channel."""
    B, C, H, W = shape
    rs = np.random.RandomState(seed + sum(shape))
    out = {"random": rs.rand(*shape) >= 0.3}
    one = np.ones((B, 1, H, W), bool)
    corner = one.copy()
    corner[:, :, 0, 0] = False                               # the clamp: un-counts four Sobel outputs per plane
    rect = one.copy()
    rect[:, :, : H // 2 + 1, W - 2:] = False                 # touches the top and the right border
    single = ~one
    single[:, :, H // 2, W // 2] = True
    single[1:] = False                                       # ONE valid pixel in the whole call
    out.update(corner=corner, rect=rect, single=single, none=~one)
    if B > 1:
        sample = one.copy()
        sample[0] = False                                    # one whole sample void
        sample[1:, :, 2, 1] = False
        out["sample"] = sample
    return out


def pair(shape):
    p, g = V.pair(190 + sum(shape), shape)
    return torch.from_numpy(p), torch.from_numpy(g)


def run(crit, p, g, v, up=1.0):
    """-> ({key: 0-d device tensor}, gradient) of a Criterion / MultiLoss / LossTerm call on the GPU."""
    x = p.cuda().requires_grad_()
    out = crit(x, g.cuda(), valid=v) if v is not None else crit(x, g.cuda())
    if not isinstance(out, dict):
        out = {"Total": out}
    (up * out["Total"]).backward()
    return {k: t.detach().clone() for k, t in out.items()}, x.grad.clone()


def dev(v, dtype=torch.bool):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda().to(dtype)


def census():
    from jspsr_amd import _lib
    lib = _lib.load()
    return {k: lib.jspsr_launch_count(k.encode()) for k in KERNELS}


@pytest.mark.parametrize("shape", SHAPES)
def test_multiloss_matches_the_restatement(shape):
    from jspsr_amd.losses import MultiLoss
    p, g = pair(shape)
    for name, v in planes(shape).items():
        ref, rg = V.values_and_grad({"L1": 1.0, "L2": 1.0, "Grad": 0.1}, p, g, v, up=3.0)
        out, gr = run(MultiLoss(1.0, 1.0, 0.1), p, g, dev(v), up=3.0)
        for k in ("L1", "L2", "Grad", "Total"):
            print(shape, name, k, out[k].item(), ref[k])
            assert abs(out[k].item() - ref[k]) < 2e-6 * max(1.0, abs(ref[k])), (shape, name, k, out[k].item(), ref[k])
        err = (gr.cpu().double() - rg).abs().max().item()
        print(shape, name, "grad err", err, rg.abs().max().item())
        assert err < 1e-6 * rg.abs().max().item() + 1e-9, (shape, name, err)


@pytest.mark.parametrize("shape", SHAPES)
def test_menu_terms_and_five_key_criterion_match_the_restatement(shape):
    from jspsr_amd.losses import get_criterion, get_loss
    p, g = pair(shape)
    for name, v in planes(shape).items():
        for term in ("berhu", "bce", "norm"):
            if term == "norm" and shape[1] != 1:
                continue
            ref, rg = V.values_and_grad({term: 1.0}, p, g, v)
            out, gr = run(get_loss(term), p, g, dev(v, torch.uint8))
            scale = rg.abs().max().item()
            print(shape, name, term, out["Total"].item(), ref["Total"], scale)
            assert abs(out["Total"].item() - ref["Total"]) <= 1e-5 * abs(ref["Total"]) + 1e-7, (shape, name, term)
            err = (gr.cpu().double() - rg).abs().max().item()
            assert err <= 1e-5 * scale + 1e-12, (shape, name, term, err, scale)
        ref, rg = V.values_and_grad(FIVE, p, g, v, up=2.0)
        out, gr = run(get_criterion(FIVE), p, g, dev(v), up=2.0)
        assert list(out) == list(FIVE) + ["Total"]
        for k in FIVE:
            tol = 2e-6 * max(1.0, abs(ref[k])) if k.lower() in BASE else 1e-5 * abs(ref[k]) + 1e-7
            assert abs(out[k].item() - ref[k]) <= tol, (shape, name, k, out[k].item(), ref[k])
        total = sum(w * out[k].double().item() for k, w in FIVE.items())
        assert out["Total"].item() == np.float32(total), (shape, name)                  # in double, rounded once
        scale = rg.abs().max().item()
        err = (gr.cpu().double() - rg).abs().max().item()
        assert err <= 1e-6 * scale + 1e-9 + 1e-5 * scale + 1e-12, (shape, name, err, scale)


@pytest.mark.parametrize("shape", SHAPES + [(2, 1, 96, 130)])
def test_all_ones_plane_has_the_bits_of_the_unmasked_call(shape):
    from jspsr_amd.losses import MultiLoss, get_criterion, get_loss
    p, g = pair(shape)
    crits = [MultiLoss(1, 1, 0.1), get_criterion(FIVE), get_loss("berhu")] + ([get_loss("norm")] if shape[1] == 1 else [])
    B, C, H, W = shape
    for crit in crits:
        want, wg = run(crit, p, g, None, up=1.5)
        for ones in (torch.ones((B, 1, H, W), dtype=torch.bool, device="cuda"),
                     torch.full(shape, 255, dtype=torch.uint8, device="cuda")):
            got, gg = run(crit, p, g, ones, up=1.5)
            assert list(got) == list(want)
            assert all(torch.equal(got[k], want[k]) for k in want), (shape, str(crit), {k: (got[k].item(), want[k].item()) for k in want})
            assert torch.equal(gg, wg), (shape, str(crit), (gg - wg).abs().max().item())


@pytest.mark.parametrize("shape", SHAPES)
def test_what_the_rasters_hold_at_masked_elements_has_no_influence(shape):
    from jspsr_amd.losses import MultiLoss, get_criterion
    p, g = pair(shape)
    for name, v in planes(shape).items():
        full = np.broadcast_to(v, shape)
        inv = torch.from_numpy(~full)
        for crit in (MultiLoss(1, 1, 0.1), get_criterion(FIVE)):
            want, wg = run(crit, p, g, dev(v))
            assert all(torch.isfinite(t).all() for t in want.values()) and torch.isfinite(wg).all(), (shape, name)
            # +0.0 at every invalid element: all 32 bits clear
            assert not wg.cpu().view(torch.int32)[inv].any(), (shape, name)
            again, ag = run(crit, p, g, dev(v))                                      # two runs, the same bits
            assert all(torch.equal(again[k], want[k]) for k in want) and torch.equal(ag, wg)
            for i, junk in enumerate(JUNK):
                p2, g2 = p.clone(), g.clone()
                p2[inv] = junk
                g2[inv] = JUNK[(i + 1) % len(JUNK)]
                got, gg = run(crit, p2, g2, dev(v, torch.uint8) * 7)                 # any non-zero byte is valid
                assert all(torch.equal(got[k], want[k]) for k in want), (shape, name, junk)
                assert torch.equal(gg.cpu().view(torch.int32), wg.cpu().view(torch.int32)), (shape, name, junk)


@pytest.mark.parametrize("shape", SHAPES)
def test_nothing_valid_gives_zero_not_nan(shape):
    from jspsr_amd.losses import MultiLoss, get_criterion, get_loss
    p, g = pair(shape)
    p[0, 0, 0, 0], g[0, 0, 1, 1] = float("nan"), -32767.0
    none = torch.zeros(shape, dtype=torch.bool, device="cuda")
    crits = [MultiLoss(1, 1, 0.1), get_criterion(FIVE), get_loss("bce")] + ([get_criterion({"Norm": 1, "L2": 2})] if shape[1] == 1 else [])
    for crit in crits:
        out, gr = run(crit, p, g, none)
        assert all(t.item() == 0.0 for t in out.values()), (shape, str(crit), out)
        assert not gr.cpu().view(torch.int32).any(), (shape, str(crit))


def test_masked_criterion_captures_in_a_graph():
    """Forward + backward captured; a replay after the PLANE's contents (and pred) change in place equals the eager result
    bit for bit: N, N_g and BerHu's threshold are recomputed on the device."""
    from jspsr_amd.losses import get_criterion
    crit = get_criterion(FIVE)
    shape = (2, 1, 64, 80)
    p0, g0 = pair(shape)
    p1 = V.pair(7, shape)[0] * 1.5 - 0.1
    rs = np.random.RandomState(5)
    v0, v1 = rs.rand(2, 1, 64, 80) >= 0.3, rs.rand(2, 1, 64, 80) >= 0.6
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
        x.copy_(torch.from_numpy(p1).cuda())
        plane.copy_(dev(v1, torch.uint8))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: t.clone() for k, t in out.items()}
    got_g = x.grad.clone()
    ref, ref_g = run(crit, torch.from_numpy(p1), g0, dev(v1, torch.uint8))
    assert all(torch.equal(got[k].detach(), ref[k]) for k in ref), {k: (got[k].item(), ref[k].item()) for k in ref}
    assert torch.equal(got_g, ref_g)
    assert not got_g[1].any() and got_g[0].any()


def test_refusals_before_any_launch():
    from jspsr_amd.losses import MultiLoss, get_criterion, get_loss
    x = torch.rand(2, 1, 16, 20, device="cuda")
    ok = torch.ones(2, 1, 16, 20, dtype=torch.bool, device="cuda")
    c0 = census()
    for crit in (get_loss("ssim"), get_criterion({"L1": 1, "SSIM": 0.5})):
        with pytest.raises(NotImplementedError, match="SSIM"):
            crit(x, x, valid=ok)
    for crit in (MultiLoss(1, 1, 0.1), get_criterion(FIVE), get_loss("l1")):
        for bad in (ok[:1], ok[:, :, :15], ok[0], ok.expand(2, 3, 16, 20), ok.reshape(2, 1, 20, 16)):
            with pytest.raises(ValueError, match="valid"):
                crit(x, x, valid=bad)
        for bad in (ok.float(), ok.to(torch.int32), ok.cpu().numpy()):
            with pytest.raises(TypeError, match="valid"):
                crit(x, x, valid=bad)
        with pytest.raises(ValueError, match="valid"):
            crit(x, x, valid=ok.cpu())
    assert census() == c0
