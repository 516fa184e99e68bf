"""GPU: the loss menu (jspsr_loss_menu_*, jspsr_ssim_*; csrc/loss_terms.hip) through jspsr_amd.losses.get_loss /
get_criterion and jspsr_amd.metrics.ssim / Meter(ssim=...), against the fp64 restatements of tests/loss_menu_ref.py and
the reference-made fixture tests/golden/g10_loss_menu.npz."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import jspsr_ref as R
from tests import fixtures as Fx
from tests import loss_menu_ref as M

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_loss_menu.npz")
KERNELS = ("loss_forward", "loss_finalize", "loss_backward", "loss_menu_max", "loss_menu_sum", "ssim_forward",
           "loss_menu_combine", "loss_menu_backward", "ssim_backward", "ssim_finalize")
SHAPES = [(1, 1, 11, 11), (2, 1, 11, 40), (1, 1, 37, 61), (2, 3, 45, 70), (8, 1, 512, 512)]
FIVE = {"L1": 1, "L2": 1, "Grad": 0.1, "SSIM": 0.5, "Berhu": 0.2}


def _census():
    from jspsr_amd import _lib
    lib = _lib.load()
    return {k: lib.jspsr_launch_count(k.encode()) for k in KERNELS}


def _delta(a, b):
    return {k: b[k] - a[k] for k in KERNELS if b[k] != a[k]}


def _pair(shape, seed):
    p, g = M.dem_pair(seed, shape)
    return torch.from_numpy(p), torch.from_numpy(g)


def _gpu(fn, p, g):
    x = p.cuda().requires_grad_()
    v = fn(x, g.cuda())
    v.backward()
    torch.cuda.synchronize()
    return v.item(), x.grad.cpu().double()


def _tolerances(name, p, g):
    """fp64 value / gradient and tolerances: for SSIM from the fp32 torch restatement's own deviation from fp64."""
    v64, g64 = M.value_and_grad(M.TERMS[name], p, g)
    scale = g64.abs().max().item()
    if name != "ssim":
        return v64, g64, 1e-5 * abs(v64) + 1e-7, 1e-5 * scale + 1e-12
    x = p.clone().requires_grad_()
    v32 = M.TERMS[name](x, g)
    v32.backward()
    dv = abs(v32.item() - v64)
    dg = (x.grad.double() - g64).abs().max().item()
    return v64, g64, 4 * dv + 1e-6, 4 * dg + 1e-4 * scale


@pytest.mark.parametrize("name", ["l1", "l2", "bce", "berhu", "norm", "ssim"])
def test_each_term_alone_matches_restatement(name):
    from jspsr_amd.losses import get_loss
    for i, shape in enumerate(SHAPES):
        if name == "norm" and shape[1] != 1:
            continue
        p, g = _pair(shape, 100 + i)
        v, gr = _gpu(get_loss(name), p, g)
        v64, g64, tv, tg = _tolerances(name, p, g)
        assert abs(v - v64) <= tv, (name, shape, v, v64, tv)
        err = (gr - g64).abs().max().item()
        assert err <= tg, (name, shape, err, tg)


def test_fixture_terms_and_reference_criteria():
    from jspsr_amd.losses import get_criterion, get_loss
    z = np.load(FIX)
    p, g = torch.from_numpy(z["pred"]), torch.from_numpy(z["gt"])
    for name in ("l1", "l2", "mse", "bce", "vanilla", "berhu", "norm"):
        v, gr = _gpu(get_loss(name), p, g)
        ref_v, ref_g = float(z[f"{name}_value"]), torch.from_numpy(z[f"{name}_grad"])
        assert abs(v - ref_v) <= 1e-5 * abs(ref_v), (name, v, ref_v)
        assert (gr - ref_g).abs().max().item() <= 1e-5 * ref_g.abs().max().item() + 1e-9, name
    # the reference MultiLoss with non-unit weights, and its SingleLoss
    keys = [str(k) for k in z["multi_keys"]]
    crit = get_criterion(dict(zip(keys[:-1], z["multi_weights"].tolist())))
    x = p.cuda().requires_grad_()
    out = crit(x, g.cuda())
    assert list(out) == keys and all(not out[k].requires_grad for k in keys[:-1]) and out["Total"].requires_grad
    out["Total"].backward()
    got = [out[k].item() for k in keys]
    assert np.allclose(got, z["multi_values"], rtol=1e-5, atol=0), (got, z["multi_values"])
    ref_g = torch.from_numpy(z["multi_grad"])
    assert (x.grad.cpu().double() - ref_g).abs().max().item() <= 1e-5 * ref_g.abs().max().item()
    single = get_criterion({"Berhu": 7.0})
    x = p.cuda().requires_grad_()
    out = single(x, g.cuda())
    out["Total"].backward()
    assert list(out) == ["Berhu", "Total"] and out["Berhu"].item() == out["Total"].item()
    assert np.allclose([out["Berhu"].item()], z["single_values"][:1], rtol=1e-5)
    ref_g = torch.from_numpy(z["single_grad"])
    assert (x.grad.cpu().double() - ref_g).abs().max().item() <= 1e-5 * ref_g.abs().max().item()


def test_berhu_at_equal_inputs_is_zero_with_zero_gradient():
    from jspsr_amd.losses import get_loss
    g = _pair((2, 1, 20, 33), 7)[1]
    v, gr = _gpu(get_loss("berhu"), g.clone(), g)
    assert v == 0.0 and torch.count_nonzero(gr).item() == 0        # the reference's gradient here is NaN


def test_ssim_meter_values():
    from jspsr_amd.metrics import Meter, local_window, prepare, ssim
    z = np.load(FIX)
    for i in range(len(M.SSIM_SHAPES)):
        p, g = (torch.from_numpy(a) for a in M.ssim_inputs(i))
        v = ssim(p.cuda(), g.cuda(), "local").item()
        v64 = M.ssim_local(g.double(), p.double(), local_window().double()).item()
        v32 = M.ssim_local(g, p, local_window()).item()
        assert abs(v - float(z[f"ssim_local_{i}"])) <= 1e-6 + 4 * abs(v32 - v64), (i, v, float(z[f"ssim_local_{i}"]))
        vp = ssim(p.cuda(), g.cuda(), "piq").item()
        vp64 = M.ssim_piq(g.double(), p.double()).item()
        assert abs(vp - vp64) <= 1e-6 + 4 * abs(M.ssim_piq(g, p).item() - vp64), (i, vp, vp64)
    # Meter: without ssim exactly today's keys and values; with it, "SSIM" after the same prepare()
    tiles = [_pair((1, 1, 100, 120), 300 + i) for i in range(3)]
    base, local, piq = Meter(-80.0, 929.0), Meter(-80.0, 929.0, ssim="local"), Meter(-80.0, 929.0, ssim="piq")
    for p, g in tiles:
        for m in (base, local, piq):
            m.update(p.cuda(), g.cuda())
    s0, s1, s2 = base.scores(), local.scores(), piq.scores()
    assert list(s0) == list(Meter.NAMES) and list(s1) == list(Meter.NAMES) + ["SSIM"]
    assert all(s0[k] == s1[k] == s2[k] for k in Meter.NAMES)
    for pk, s in (("local", s1), ("piq", s2)):
        want = np.mean([ssim(*[t.contiguous() for t in prepare(p.cuda(), g.cuda(), 0.05)], pk).item() for p, g in tiles])
        assert abs(s["SSIM"] - want) <= 1e-6, (pk, s["SSIM"], want)


def test_default_config_is_bit_identical_to_multiloss():
    from jspsr_amd.losses import MultiLoss, get_criterion
    p, g = (t.cuda() for t in _pair((2, 1, 96, 130), 11))
    x1, x2 = p.clone().requires_grad_(), p.clone().requires_grad_()
    ref = MultiLoss(1, 1, 0.1)(x1, g)
    ref["Total"].backward()
    c0 = _census()
    out = get_criterion({"L1": 1, "L2": 1, "Grad": 0.1})(x2, g)
    out["Total"].backward()
    torch.cuda.synchronize()
    assert _delta(c0, _census()) == {"loss_forward": 1, "loss_finalize": 1, "loss_backward": 1}
    assert list(out) == ["L1", "L2", "Grad", "Total"]
    assert all(torch.equal(out[k], ref[k]) for k in out)
    assert torch.equal(x1.grad, x2.grad)


def test_five_term_criterion():
    from jspsr_amd.losses import get_criterion
    p, g = (t.cuda() for t in _pair((2, 1, 75, 90), 12))
    crit = get_criterion(FIVE)
    runs = []
    for _ in range(2):
        x = p.clone().requires_grad_()
        c0 = _census()
        out = crit(x, g)
        c1 = _census()
        out["Total"].backward()
        c2 = _census()
        runs.append(({k: v.clone() for k, v in out.items()}, x.grad.clone()))
        assert sum(_delta(c0, c1).values()) <= 6 and sum(_delta(c1, c2).values()) <= 3, (_delta(c0, c1), _delta(c1, c2))
    (o1, g1), (o2, g2) = runs
    assert all(torch.equal(o1[k], o2[k]) for k in o1) and torch.equal(g1, g2)      # the same bits on every run
    assert list(o1) == list(FIVE) + ["Total"]
    total = sum(w * o1[k].double().item() for k, w in FIVE.items())
    assert o1["Total"].item() == np.float32(total), (o1["Total"].item(), total)
    from jspsr_amd.losses import get_loss
    gsum = torch.zeros_like(p, dtype=torch.float64)
    for k, w in FIVE.items():
        x = p.clone().requires_grad_()
        v = get_loss(k)(x, g)
        v.backward()
        assert abs(v.item() - o1[k].item()) <= 1e-6 * abs(v.item()), k
        gsum += w * x.grad.double()
    assert (g1.double() - gsum).abs().max().item() <= 1e-5 * gsum.abs().max().item()


def test_criterion_captures_in_a_graph():
    """Forward + backward captured; a replay after pred changes in place equals the eager result bit for bit (BerHu's
    threshold is recomputed on the device)."""
    from jspsr_amd.losses import get_criterion
    crit = get_criterion(FIVE)
    p0, g0 = _pair((2, 1, 64, 80), 13)
    p1 = _pair((2, 1, 64, 80), 14)[0] * 1.5 - 0.1                       # a different max|pred - gt|
    g = g0.cuda()
    x = p0.cuda().requires_grad_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                               # warm up off the capture
            x.grad = None
            crit(x, g)["Total"].backward()
    torch.cuda.current_stream().wait_stream(s)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crit(x, g)
        out["Total"].backward()
    with torch.no_grad():
        x.copy_(p1.cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in out.items()}
    got_g = x.grad.clone()
    xe = p1.cuda().requires_grad_()
    ref = crit(xe, g)
    ref["Total"].backward()
    assert all(torch.equal(got[k], ref[k]) for k in ref), {k: (got[k].item(), ref[k].item()) for k in ref}
    assert torch.equal(got_g, xe.grad)


def test_error_paths():
    from jspsr_amd import _lib
    from jspsr_amd.losses import get_criterion, get_loss
    from jspsr_amd.metrics import ssim
    c0 = _census()
    for shape in ((1, 1, 10, 40), (1, 1, 40, 10)):
        x = torch.rand(shape, device="cuda")
        with pytest.raises(ValueError, match="SSIM"):
            get_loss("ssim")(x, x)
        with pytest.raises(ValueError):
            ssim(x, x, "piq")
    x = torch.rand(1, 2, 16, 16, device="cuda")
    with pytest.raises(ValueError, match="Norm"):
        get_criterion({"Norm": 1, "Berhu": 1})(x, x)
    assert _delta(c0, _census()) == {}
    lib = _lib.load()
    EINVAL = -1
    buf = torch.zeros(1 << 20, device="cuda")
    ptr, s = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    slots, w = (ctypes.c_int * 1)(6), (ctypes.c_double * 1)(1.0)
    sw = (ctypes.c_double * 7)(*[1.0] * 7)
    assert lib.jspsr_loss_menu_workspace_bytes(8, 1, 10, 64) == 0
    assert lib.jspsr_loss_menu_forward(ptr, ptr, 8, 1, 10, 64, 1, slots, w, None, ptr, ptr, s) == EINVAL
    assert lib.jspsr_loss_menu_backward(ptr, ptr, 8, 1, 64, 10, sw, None, ptr, ptr, s) == EINVAL
    assert lib.jspsr_loss_menu_forward(ptr, ptr, 1, 1, 32, 32, 1, slots, w, None, ptr, ptr, s) == EINVAL  # slot 6 not in terms
    assert lib.jspsr_loss_menu_forward(ptr, ptr, 1, 0, 32, 32, 1, slots, w, None, ptr, ptr, s) == EINVAL
    assert lib.jspsr_loss_menu_forward(None, ptr, 1, 1, 32, 32, 1, slots, w, None, ptr, ptr, s) == EINVAL
    assert lib.jspsr_loss_menu_forward(ptr, ptr, 32, 1, 32, 32, 1, slots, w, None, ptr, ptr, s) == EINVAL   # unknown term bit
    assert lib.jspsr_ssim_workspace_bytes(1, 10, 10, 0) == 0 and lib.jspsr_ssim_workspace_bytes(1, 10, 10, 1) > 0
    assert lib.jspsr_ssim_forward(ptr, ptr, 1, 10, 30, 0, None, ptr, ptr, s) == EINVAL
    assert lib.jspsr_ssim_forward(ptr, ptr, 0, 30, 30, 1, None, ptr, ptr, s) == EINVAL
    assert _delta(c0, _census()) == {}


def test_training_smoke_with_menu_criterion():
    from jspsr_amd.ddp import GradReducer
    from jspsr_amd.JSPSR import Model
    from jspsr_amd.losses import get_criterion
    from jspsr_amd.optim import FlatAdamW
    m = Model(dict(Fx.MSK, COP30=1), num_feature=8)
    m.load_state_dict(R.make_state_dict(R.jspsr_param_shapes(Fx.MSK, 8), seed=81))
    m = m.cuda().train()
    red = GradReducer(m.parameters())
    if hasattr(m, "side_streams"):
        red.watch_streams(m.side_streams("cuda"))
    opt = FlatAdamW(red, lr=1e-3, weight_decay=1e-6)
    cfg = {"L1": 1, "SSIM": 0.5, "Berhu": 0.2}
    crit = get_criterion(cfg)
    inputs, gt = R.synthetic_batch(2, 64, 64, True, seed=82)
    inputs, gt = [t.cuda() for t in inputs], gt.cuda()
    losses = []
    for step in range(5):
        red.zero_grad()
        crit.reset()
        pred = m(*inputs)
        pred.retain_grad()
        out = crit(pred, gt)
        out["Total"].backward()
        if step == 0:
            p64 = pred.detach().cpu().double().requires_grad_()
            g64 = gt.cpu().double()
            ref = sum(w * M.TERMS[k.lower()](p64, g64) for k, w in cfg.items())
            ref.backward()
            assert abs(out["Total"].item() - ref.item()) <= 1e-5 * abs(ref.item())
            err = (pred.grad.cpu().double() - p64.grad).abs().max().item()
            assert err <= 1e-4 * p64.grad.abs().max().item(), err
        red.finish()
        opt.step()
        losses.append(out["Total"].item())
    assert all(np.isfinite(losses)), losses
