"""GPU: K1p, the plain 3x3 one-channel output head (jspsr_conv_head1_*), against fp64 F.conv2d on the CPU, and the two
plain-head models (JSPSR spn=False, EDSR spn=False) against fixtures made by the reference's own modules."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import jspsr_ref as R
from tests import fixtures as Fx
from tests import plain_head_ref as P
from tests.test_secondary_models_gpu import _check


def _count(name):
    from jspsr_amd import _lib
    return _lib.load().jspsr_launch_count(name.encode())


def _raw(x_wide, coff, C, w, b, dy, dx_wide, dx_coff):
    """The C ABI on explicit (pitch, offset) operands: -> y, dw, db (dx written into dx_wide's slice)."""
    from jspsr_amd import _lib, kernels as K
    lib = _lib.load()
    B, H, W, cs = x_wide.shape
    s = torch.cuda.current_stream().cuda_stream
    y = torch.empty((B, 1, H, W), dtype=torch.float32, device="cuda")
    _lib.check(lib.jspsr_conv_head1_forward(K._dt(x_wide), x_wide.data_ptr(), cs, coff, C, w.data_ptr(), b.data_ptr(),
                                            y.data_ptr(), B, H, W, s), "forward")
    dw = torch.empty((1, C, 3, 3), dtype=torch.float32, device="cuda")
    db = torch.empty(1, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.jspsr_conv_head1_workspace_bytes(B, H, W, C), dtype=torch.uint8, device="cuda")
    _lib.check(lib.jspsr_conv_head1_backward(K._dt(x_wide), dy.data_ptr(), x_wide.data_ptr(), cs, coff, C, w.data_ptr(),
                                             dx_wide.data_ptr() if dx_wide is not None else None,
                                             dx_wide.shape[3] if dx_wide is not None else 0, dx_coff, dw.data_ptr(),
                                             db.data_ptr(), ws.data_ptr(), B, H, W, s), "backward")
    return y, dw, db


def _ref(x64, w, b, dy):
    x64 = x64.clone().requires_grad_()
    w64, b64 = w.double().cpu().requires_grad_(), b.double().cpu().requires_grad_()
    y = F.conv2d(x64, w64, b64, 1, 1)
    y.backward(dy.double().cpu())
    return y.detach(), x64.grad, w64.grad, b64.grad


SHAPES = [(1, 1, 1), (1, 3, 5), (1, 37, 61), (2, 256, 512)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [8, 16, 32, 64, 128, 256])
def test_head1_kernel_matches_fp64_conv(C, dtype):
    g = torch.Generator().manual_seed(C)
    pad = 8                                       # x and dx are channel slices [pad, pad + C) of wider buffers
    for (B, H, W) in SHAPES:
        if (B, H, W) == (2, 256, 512) and C not in (8, 64, 256):
            continue
        xw = torch.randn(B, H, W, C + 2 * pad, generator=g).to(dtype)
        w = (torch.randn(1, C, 3, 3, generator=g) / (3 * C ** 0.5)).cuda()
        b = torch.randn(1, generator=g).cuda()
        dy = torch.randn(B, 1, H, W, generator=g).cuda()
        xw = xw.cuda()
        dxw = torch.full((B, H, W, C + 2 * pad), 7.0, dtype=dtype, device="cuda")
        y, dw, db = _raw(xw, pad, C, w, b, dy, dxw, pad)
        torch.cuda.synchronize()
        x64 = xw[..., pad:pad + C].double().cpu().permute(0, 3, 1, 2)      # (bf16-rounded) inputs, exactly
        yr, dxr, dwr, dbr = _ref(x64, w, b, dy)
        tag = (C, dtype, B, H, W)
        assert y.dtype == torch.float32
        assert (y.double().cpu() - yr).abs().max().item() <= 2e-6 * yr.abs().max().item() + 1e-7, tag
        assert Fx.rel(dw, dwr) <= 1e-5 and Fx.rel(db, dbr) <= 1e-5, tag
        dx = dxw[..., pad:pad + C].double().cpu().permute(0, 3, 1, 2)
        err = (dx - dxr).abs()
        if dtype == torch.float32:
            assert err.max().item() <= 1e-5 * dxr.abs().max().item(), tag
        else:                                     # one bf16 rounding of the fp32 result (half an ulp, 2^-9 relative)
            assert (err <= 2.0 ** -8 * dxr.abs() + 1e-6 * dxr.abs().max()).all(), tag
        # nothing outside the slice was written
        assert (dxw[..., :pad] == 7).all() and (dxw[..., pad + C:] == 7).all(), tag
        # dW / db: the same bits from run to run
        _, dw2, db2 = _raw(xw, pad, C, w, b, dy, None, 0)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), tag


def test_head1_op_autograd_on_a_dense_tensor():
    from jspsr_amd import ops
    x = torch.randn(2, 9, 13, 24, device="cuda", requires_grad=True)
    w = torch.nn.Parameter(torch.randn(1, 24, 3, 3, device="cuda") * 0.1)
    b = torch.nn.Parameter(torch.randn(1, device="cuda"))
    y = ops.conv_head1(x, w, b)
    probe = torch.randn_like(y)
    (y * probe).sum().backward()
    yr, dxr, dwr, dbr = _ref(x.detach().double().cpu().permute(0, 3, 1, 2), w.detach(), b.detach(), probe)
    assert (y.detach().double().cpu() - yr).abs().max().item() <= 2e-6 * yr.abs().max().item()
    assert Fx.rel(x.grad.permute(0, 3, 1, 2), dxr) < 1e-5 and Fx.rel(w.grad, dwr) < 1e-5 and Fx.rel(b.grad, dbr) < 1e-5


# ---- the models against the reference-made fixtures ------------------------------------------------------------------
def _load(golden_dir, name, shapes, with_mask):
    z = Fx.load(golden_dir, name)
    sd, inputs, gt = Fx.regen(z, shapes, with_mask)
    return z, Fx.as_f32(sd), [t.float().cuda() for t in inputs], gt.float().cuda(), (sd, inputs)


@pytest.mark.parametrize("name,ic", [("g9_jspsr_img_nf8_b2_48x64_train.npz", Fx.IMG),
                                     ("g9_jspsr_msk_nf8_b2_64_eval.npz", Fx.MSK),
                                     ("g9_jspsr_msk_nf32_b1_64_train.npz", Fx.MSK)])
def test_jspsr_plain(golden_dir, name, ic):
    from jspsr_amd.JSPSR import Model
    nf = int(Fx.load(golden_dir, name)["nf"])
    z, sd, inputs, gt, ref64 = _load(golden_dir, name, P.jspsr_plain_param_shapes(ic, nf), "mask" in ic)
    m = Model(dict(ic, COP30=1), num_feature=nf, spn=False)
    m.load_state_dict(sd)
    m = m.cuda().train(bool(z["training"]))
    _check(z, m, m(*inputs), gt, lambda sd_, inp: P.jspsr_plain_forward(sd_, inp, True), ref64)
    if not bool(z["training"]):
        with torch.no_grad():                     # inference path: BatchNorm folded into the conv epilogues
            _check(z, m, m(*inputs), gt)


def test_edsr_plain(golden_dir):
    from jspsr_amd.EDSR import EDSR
    z, sd, inputs, gt, ref64 = _load(golden_dir, "g9_edsr_b2_40x56_train.npz", P.edsr_plain_param_shapes(4, 4, 32), False)
    m = EDSR(in_channels=4, out_channels=1, n_resblocks=4, n_features=32, scale=1)
    m.load_state_dict(sd)
    m = m.cuda().train()
    _check(z, m, m(torch.cat(inputs, 1)), gt,
           lambda sd_, inp: P.edsr_plain_forward(sd_, torch.cat(inp, 1), True, n_resblocks=4), ref64)


# ---- launch census and the fp32 prediction under bf16 -----------------------------------------------------------------
OTHER_HEADS = ["head_forward", "head_backward", "head_dbias_fold"] + [
    f"prop_{k}{s}" for k in ("forward", "backward", "head_forward", "head_backward", "logits_forward", "logits_backward",
                             "step_forward", "step_backward") for s in ("", " (dma)")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_jspsr_plain_launch_census_and_fp32_prediction(dtype, monkeypatch):
    from jspsr_amd import engine as E
    from jspsr_amd.JSPSR import Model
    sd = R.make_state_dict(P.jspsr_plain_param_shapes(Fx.MSK, 8), seed=41)
    m = Model(dict(Fx.MSK, COP30=1), num_feature=8, spn=False)
    m.load_state_dict(sd)
    m = m.cuda().train()
    m.compute_dtype = dtype
    inputs, _ = R.synthetic_batch(2, 64, 64, True, seed=42)
    inputs = [t.cuda() for t in inputs]
    seen = []
    real = E.conv_head1
    monkeypatch.setattr(E, "conv_head1", lambda x, w, b: seen.append(x.detach().clone()) or real(x, w, b))
    before = {k: _count(k) for k in ["head1_forward", "head1_backward"] + OTHER_HEADS}
    pred = m(*inputs)
    (pred * torch.randn_like(pred)).mean().backward()
    torch.cuda.synchronize()
    after = {k: _count(k) for k in before}
    assert after["head1_forward"] - before["head1_forward"] == 1
    assert after["head1_backward"] - before["head1_backward"] == 1
    assert all(after[k] == before[k] for k in OTHER_HEADS), {k: after[k] - before[k] for k in OTHER_HEADS}
    assert pred.dtype == torch.float32 and len(seen) == 1 and seen[0].dtype == dtype
    head = m.postprocessor.conv[0]
    ref = F.conv2d(seen[0].double().cpu().permute(0, 3, 1, 2), head.weight.detach().double().cpu(),
                   head.bias.detach().double().cpu(), 1, 1)
    assert (pred.detach().double().cpu() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


# ---- training and capture ---------------------------------------------------------------------------------------------
def _models():
    from jspsr_amd.EDSR import EDSR
    from jspsr_amd.JSPSR import Model
    j = Model(dict(Fx.MSK, COP30=1), num_feature=8, spn=False)
    j.load_state_dict(R.make_state_dict(P.jspsr_plain_param_shapes(Fx.MSK, 8), seed=51))
    e = EDSR(in_channels=4, out_channels=1, n_resblocks=4, n_features=32, scale=1)
    e.load_state_dict(R.make_state_dict(P.edsr_plain_param_shapes(4, 4, 32), seed=52))
    return [("jspsr", j), ("edsr", e)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plain_models_train_one_eager_step(dtype):
    from jspsr_amd.ddp import GradReducer
    from jspsr_amd.losses import MultiLoss
    from jspsr_amd.optim import FlatAdamW
    inputs, gt = R.synthetic_batch(2, 64, 64, True, seed=53)
    inputs, gt = [t.cuda() for t in inputs], gt.cuda()
    for name, m in _models():
        m = m.cuda().train()
        m.compute_dtype = dtype
        red = GradReducer(m.parameters())
        if hasattr(m, "side_streams"):
            red.watch_streams(m.side_streams("cuda"))
        opt = FlatAdamW(red, lr=1e-3, weight_decay=1e-6)
        crit = MultiLoss(1.0, 1.0, 0.1)
        before = {k: v.detach().clone() for k, v in m.named_parameters()}
        args = inputs if name == "jspsr" else [torch.cat(inputs[:2], 1)]
        red.zero_grad()
        pred = m(*args)
        assert pred.dtype == torch.float32 and pred.shape == gt.shape
        loss = crit(pred, gt)["Total"]
        loss.backward()
        red.finish()
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        head = "postprocessor.conv.0.weight" if name == "jspsr" else "head.weight"
        p = dict(m.named_parameters())
        assert not torch.equal(p[head].detach(), before[head]), (name, dtype)
        assert all(torch.isfinite(v).all() for v in p.values())


def test_graphed_step_is_bit_identical_to_the_eager_step_plain():
    from jspsr_amd.ddp import GradReducer
    from jspsr_amd.graph import GraphedStep
    from jspsr_amd.JSPSR import Model
    from jspsr_amd.losses import MultiLoss
    from jspsr_amd.optim import FlatAdamW
    sd = R.make_state_dict(P.jspsr_plain_param_shapes(Fx.MSK, 8), seed=61)
    batches = []
    for s in range(2):
        inp, gt = R.synthetic_batch(2, 64, 64, True, seed=62 + s)
        batches.append(([t.cuda() for t in inp], gt.cuda()))

    def build(dtype):
        m = Model(dict(Fx.MSK, COP30=1), num_feature=8, spn=False)
        m.load_state_dict(sd)
        m = m.cuda().train()
        m.compute_dtype = dtype
        red = GradReducer(m.parameters())
        red.watch_streams(m.side_streams("cuda"))
        return m, red, FlatAdamW(red, lr=1e-3, weight_decay=1e-6), MultiLoss(1.0, 1.0, 0.1)

    for dtype in (torch.float32, torch.bfloat16):
        m, red, opt, crit = build(dtype)
        losses_e = []
        for i in range(6):
            inp, gt = batches[0 if i < 4 else 1]
            red.zero_grad()
            loss = crit(m(*inp), gt)["Total"]
            loss.backward()
            red.finish()
            opt.step()
            losses_e.append(loss.item())
        ref = {k: v.clone() for k, v in m.state_dict().items()}
        m, red, opt, crit = build(dtype)
        step = GraphedStep(m, red, opt, crit, *batches[0], warmup=3)
        losses_g = [step().item(), step(*batches[1]).item(), step().item()]
        assert losses_g == losses_e[3:], (dtype, losses_g, losses_e)
        for k, v in m.state_dict().items():
            assert torch.equal(v, ref[k]), (dtype, k)


# ---- strip inference --------------------------------------------------------------------------------------------------
def test_jspsr_plain_strips_equal_the_monolithic_forward():
    from jspsr_amd import tiling
    from jspsr_amd.JSPSR import Model
    m = Model(dict(Fx.MSK, COP30=1), num_feature=8, spn=False)
    m.load_state_dict(R.make_state_dict(P.jspsr_plain_param_shapes(Fx.MSK, 8), seed=71))
    m = m.cuda().eval()
    inputs, _ = R.synthetic_batch(1, 1024, 256, True, seed=72)
    inputs = [t.cuda() for t in inputs]
    with torch.no_grad():
        mono = m(*inputs)
    for world in (2, 4):
        out, reach = tiling.emulate_sharded_forward(m, inputs, world, halo=128, return_reach=True)
        assert reach == [0.0] * world
        assert (out - mono).abs().max().item() < 2e-5, world


def test_edsr_plain_strips_equal_the_monolithic_forward():
    from jspsr_amd import tiling
    from jspsr_amd.EDSR import EDSR
    m = EDSR(in_channels=4, out_channels=1, n_resblocks=8, n_features=32, scale=1)
    m.load_state_dict(R.make_state_dict(P.edsr_plain_param_shapes(4, 8, 32), seed=73))
    m = m.cuda().eval()
    assert m.receptive_radius == 19
    inputs, _ = R.synthetic_batch(1, 512, 128, False, seed=74)
    x = torch.cat(inputs, 1).cuda()
    with torch.no_grad():
        mono = m(x)
    for world in (2, 4):
        out = tiling.emulate_sharded_forward(m, [x], world, halo=32)
        assert (out - mono).abs().max().item() <= 1e-6 * mono.abs().max().item(), world
