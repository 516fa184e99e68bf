"""The gated ConvUnit as one autograd node (ops._GatedConvBN: the conv and its weight gradient read x through the gate's
per-image scale while they stage their operand) against the unfused composition (ops.gate_fuse off: gate_scale writes
x * s, the conv reads it) in the same process.  The staged value is the one gate_scale stores and no sum changes its
order, so everything must agree bit for bit: torch.equal, no tolerance.  Every case proves the kernel it means to test
with the launch census."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("conv_patch", "conv_patch_16x16", "conv_patch_16x16x128", "conv_igemm", "conv64_resident", "conv128_resident",
         "conv2d_wgrad_patch", "conv2d_wgrad", "gate_scale", "gate_pool")


def _counts():
    from jspsr_amd import _lib
    lib = _lib.load()
    return {n: lib.jspsr_launch_count(n.encode()) for n in NAMES}


def _delta(a, b):
    return {n: b[n] - a[n] for n in NAMES if b[n] != a[n]}


def _unit(cin, cout, seed):
    from jspsr_amd.blocks import ConvUnit
    torch.manual_seed(seed)
    m = ConvUnit(cin, cout, 3, bn=True, relu=True, gate=True)
    with torch.no_grad():      # a random MLP far from its initialisation: s spreads over (0, 1) and differs from image to image
        m.camb.fc[0].weight.normal_(0, 3.0 / cin ** 0.5)
        m.camb.fc[1].weight.normal_(0, 2.0 / (cin // 16) ** 0.5)
        m.conv.bn.weight.normal_(1.0, 0.2)
        m.conv.bn.bias.normal_(0.0, 0.2)
    return m.cuda().train()


def _inputs(B, H, W, cin, cout, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g) + 0.5 * torch.randn(B, 1, 1, cin, generator=g)   # per-image channel offsets
    dout = torch.randn(B, H, W, cout, generator=g)
    return x.cuda().to(dtype), dout.cuda().to(dtype)


def _step(m, x, dout, fuse):
    from jspsr_amd import ops
    prev, ops.gate_fuse = ops.gate_fuse, fuse
    try:
        x = x.clone().requires_grad_()
        c0 = _counts()
        out = m(x)
        c1 = _counts()
        out.backward(dout)
        torch.cuda.synchronize()
        c2 = _counts()
    finally:
        ops.gate_fuse = prev
    bn = m.conv.bn
    res = dict(out=out.detach(), dx=x.grad, dW=m.conv[0].weight.grad, dw1=m.camb.fc[0].weight.grad, dw2=m.camb.fc[1].weight.grad,
               dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean, running_var=bn.running_var,
               batches=bn.num_batches_tracked)
    return res, _delta(c0, c1), _delta(c1, c2)


def _compare(B, H, W, cin, cout, dtype):
    m = _unit(cin, cout, seed=cin + cout)
    ref = copy.deepcopy(m)
    x, dout = _inputs(B, H, W, cin, cout, dtype, seed=H * W + cin)
    got, fwd, bwd = _step(m, x, dout, True)
    want, fwd_ref, bwd_ref = _step(ref, x, dout, False)
    from jspsr_amd import kernels as K
    s = K.gate_mlp_forward(*K.gate_pool(x)[:2], m.camb.fc[0].weight.detach().float().flatten(1).contiguous(),
                           m.camb.fc[1].weight.detach().float().flatten(1).contiguous())[0]
    assert (s[0] - s[1]).abs().max().item() > 0.05 and 0.1 < s.mean().item() < 0.9, "the images' gates should differ"
    for k, v in want.items():
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(got[k], v), (k, (got[k].float() - v.float()).abs().max().item())
    assert fwd_ref.get("gate_scale") == 1 and "gate_scale" not in bwd_ref, (fwd_ref, bwd_ref)
    convs = ("conv_patch", "conv_patch_16x16", "conv_patch_16x16x128", "conv_igemm", "conv64_resident", "conv128_resident")
    assert {n: fwd.get(n) for n in convs} == {n: fwd_ref.get(n) for n in convs}, (fwd, fwd_ref)    # like against like
    return fwd, bwd


DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,cin,cout,kernel", [
    (3, 20, 24, 64, 32, "conv_patch"),              # 8x16 tiles x 32 channels, ragged edges, one bf16 channel chunk
    (3, 20, 24, 128, 64, "conv_patch"),             # 8x16 tiles x 64 channels, two chunks
    (3, 24, 40, 128, 128, "conv_patch"),            # the 128 x 128 tile
    (4, 128, 128, 64, 256, "conv_patch_16x16"),     # 256 tiles x 4 channel blocks = 1024: the smallest raster on <256,64,4,1>
    (4, 256, 256, 128, 64, "conv_patch_16x16"),     # <= 64 output channels: 16x16 tiles from 1024 tiles (conv.hip, launch());
                                                    # (128 inputs: the composition's bf16 64 -> 64 conv would go to K2r)
])
def test_fused_gated_unit_equals_the_composition(dtype, B, H, W, cin, cout, kernel):
    fwd, bwd = _compare(B, H, W, cin, cout, dtype)
    # forward: pool, MLP, ONE conv on the kernel meant, no gate_scale
    assert fwd.get(kernel) == 1 and "gate_scale" not in fwd, fwd
    assert not any(fwd.get(n) for n in ("conv_igemm", "conv64_resident", "conv128_resident")), fwd
    wide = W % (32 if dtype == torch.float32 else 64) == 0        # the nine-tap weight gradient takes whole strips only
    if wide:
        assert bwd.get("conv2d_wgrad_patch") == 1 and "gate_scale" not in bwd and "conv2d_wgrad" not in bwd, bwd
    else:                                                         # x * s is re-formed for the weight gradient alone
        assert bwd.get("conv2d_wgrad") == 1 and bwd.get("gate_scale") == 1, bwd


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_weight_gradient_with_several_row_blocks_per_image(dtype):
    """3 x 20 x 64, 64 -> 32: the nine-tap kernel's plan gives 8 rows per workgroup (its minimum), i.e. three row blocks
    per strip and one (fp32: two) strips per image -- a workgroup's image is strip / strips_x, not its block index."""
    fwd, bwd = _compare(3, 20, 64, 64, 32, dtype)
    assert fwd.get("conv_patch") == 1 and "gate_scale" not in fwd, fwd
    assert bwd.get("conv2d_wgrad_patch") == 1 and "gate_scale" not in bwd and "conv2d_wgrad" not in bwd, bwd


@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_shape_falls_back_to_the_separate_pass(dtype):
    """48 input channels are no multiple of the patch kernels' stage depth (32 fp32 / 64 bf16 channels)."""
    fwd, bwd = _compare(3, 12, 16, 48, 32, dtype)
    assert fwd.get("gate_scale") == 1 and fwd.get("conv_igemm") == 1, fwd


def test_training_step_of_a_gated_unit_launches_no_gate_scale():
    m = _unit(128, 64, seed=3)
    x, dout = _inputs(3, 16, 64, 128, 64, torch.bfloat16, seed=4)
    _, fwd, bwd = _step(m, x, dout, True)
    assert fwd.get("gate_pool") == 1 and bwd.get("conv2d_wgrad_patch") == 1, (fwd, bwd)
    assert "gate_scale" not in fwd and "gate_scale" not in bwd, (fwd, bwd)
