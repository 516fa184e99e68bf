"""GPU: the BatchNorm + residual + ReLU backward (relu mode 1) on fewer tensor passes.

The reduce pass writes the masked gradient once and the apply pass reads it back; the ReLU mask comes from one bit per
element written by the forward instead of from the saved output.  Neither changes a bit of any result: the bit-mask form is
compared with the form that reads y with torch.equal, the masked gradient with where(y > 0, dy, 0), and dx / dgamma /
dbeta with torch CPU fp64 autograd under the tolerances of test_elementwise_gpu.py::test_bn_forward_backward."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RES_SCALE = 0.5
NAMES = ("bn_bwd_reduce", "bn_bwd_finalize", "bn_bwd_apply")
# (B, H, W, C, channel pitch, channel offset): odd pixel counts in one chunk; many workgroups; channel slices of wider tensors
CASES = [(1, 7, 5, 16, 16, 0), (2, 9, 13, 64, 64, 0), (2, 64, 64, 64, 64, 0), (2, 9, 13, 64, 96, 32)]


def _k():
    from jspsr_amd import kernels
    return kernels


def _census():
    from jspsr_amd import _lib
    lib = _lib.load()
    return {n: lib.jspsr_launch_count(n.encode()) for n in NAMES}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _place(t, dtype, cs, coff):
    """NHWC fp32 CPU tensor -> device tensor of `dtype`, dense or as channels [coff, coff + C) of a buffer of pitch cs."""
    t = t.cuda().to(dtype)
    if cs == t.shape[3]:
        return t
    wide = torch.full(t.shape[:3] + (cs,), float("nan"), dtype=dtype, device="cuda")
    wide[..., coff:coff + t.shape[3]] = t
    return wide[..., coff:coff + t.shape[3]]


@functools.lru_cache(maxsize=None)
def _case(dtype, B, H, W, C, cs, coff):
    """Inputs, the fp64 autograd reference (computed once, never modified) and both forms of the backward."""
    K = _k()
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W + cs)
    x = torch.randn(B, H, W, C, generator=g) * 1.7 + 0.4
    res = torch.randn(B, H, W, C, generator=g)
    dy = torch.randn(B, H, W, C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    if dtype == torch.bfloat16:
        x, res, dy = x.bfloat16().float(), res.bfloat16().float(), dy.bfloat16().float()
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    xr, gr, br = nchw(x).requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    yr = F.relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5) * RES_SCALE + nchw(res))
    yr.backward(nchw(dy))
    ref = dict(dx=xr.grad.permute(0, 2, 3, 1), dgamma=gr.grad, dbeta=br.grad)

    xd, resd, dyd = (_place(t, dtype, cs, coff) for t in (x, res, dy))
    out = _place(torch.zeros(B, H, W, C), dtype, cs, coff)
    gd, bd = gamma.cuda(), beta.cuda()
    y, mean, invstd, mask = K.bn_forward(xd, gd, bd, None, None, 0.1, 1e-5, True, True, resd, RES_SCALE, out=out, want_mask=True)
    assert mask.dtype == torch.uint8 and y.data_ptr() == out.data_ptr()
    n0 = _census()
    from_y = K.bn_backward(dyd, y, xd, gd, mean, invstd, True, 1, RES_SCALE, want_dres=True, beta=bd)
    n1 = _census()
    from_mask = K.bn_backward(dyd, None, xd, gd, mean, invstd, True, 1, RES_SCALE, want_dres=True, beta=bd, mask=mask)
    n2 = _census()
    no_dres_y = K.bn_backward(dyd, y, xd, gd, mean, invstd, True, 1, RES_SCALE, beta=bd)
    no_dres_mask = K.bn_backward(dyd, None, xd, gd, mean, invstd, True, 1, RES_SCALE, beta=bd, mask=mask)
    n3 = _census()
    torch.cuda.synchronize()
    return dict(ref=ref, y=y, dy=dyd, from_y=from_y, from_mask=from_mask, no_dres_y=no_dres_y, no_dres_mask=no_dres_mask,
                census=(n0, n1, n2, n3))


PARAMS = [pytest.param(dt, *c, id=f"{str(dt)[6:]}-{'x'.join(map(str, c[:4]))}-pitch{c[4]}")
          for dt in (torch.float32, torch.bfloat16) for c in CASES]


@pytest.mark.parametrize("dtype,B,H,W,C,cs,coff", PARAMS)
def test_bit_mask_gives_the_bits_of_the_saved_output(dtype, B, H, W, C, cs, coff):
    c = _case(dtype, B, H, W, C, cs, coff)
    for name, a, b in zip(("dx", "dres", "dgamma", "dbeta"), c["from_y"], c["from_mask"]):
        assert torch.equal(a, b), name
    # without the residual gradient (the apply pass masks for itself): the same dx, from y and from the bit mask
    for form in ("no_dres_y", "no_dres_mask"):
        assert c[form][1] is None
        for i, name in ((0, "dx"), (2, "dgamma"), (3, "dbeta")):
            assert torch.equal(c[form][i], c["from_y"][i]), (form, name)


@pytest.mark.parametrize("dtype,B,H,W,C,cs,coff", PARAMS)
def test_masked_gradient_is_exact_and_results_match_fp64(dtype, B, H, W, C, cs, coff):
    c = _case(dtype, B, H, W, C, cs, coff)
    gtol = 1e-5 if dtype == torch.float32 else 1.5e-2          # test_bn_forward_backward's
    for form in ("from_y", "from_mask"):
        dx, dres, dgamma, dbeta = c[form]
        assert dres.is_contiguous() and dx.is_contiguous()
        assert torch.equal(dres, torch.where(c["y"] > 0, c["dy"], torch.zeros_like(c["dy"]))), form
        for name, got in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
            err = _rel(got.float().cpu(), c["ref"][name])
            print(f"{form} {name}: rel err {err:.3e} (bound {gtol:g})")
            assert err < gtol, (form, name, err)


@pytest.mark.parametrize("dtype,B,H,W,C,cs,coff", PARAMS)
def test_launch_census_is_unchanged(dtype, B, H, W, C, cs, coff):
    n0, n1, n2, n3 = _case(dtype, B, H, W, C, cs, coff)["census"]
    for n in NAMES:      # one reduce, one finalize, one apply per call, whichever form
        assert n1[n] - n0[n] == 1 and n2[n] - n1[n] == 1 and n3[n] - n2[n] == 2, (n, n0, n1, n2, n3)


def test_mask_arguments_are_checked():
    K = _k()
    x = torch.randn(1, 4, 4, 16, device="cuda")
    gamma, beta = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
    from jspsr_amd._lib import JspsrHipError
    with pytest.raises(JspsrHipError):       # a bit mask without a residual: mode 2 recomputes the mask from x instead
        K.bn_forward(x, gamma, beta, None, None, 0.1, 1e-5, True, True, want_mask=True)
    y, mean, invstd, mask = K.bn_forward(x, gamma, beta, None, None, 0.1, 1e-5, True, True, x, want_mask=True)
    with pytest.raises(ValueError):          # a mask of another shape
        K.bn_backward(x, None, x, gamma, mean, invstd, True, 1, mask=mask[:-1])
    with pytest.raises(JspsrHipError):       # neither y nor a mask
        K.bn_backward(x, None, x, gamma, mean, invstd, True, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("project", [False, True])
def test_res_unit_gradients_do_not_depend_on_the_switch(dtype, project, monkeypatch):
    from jspsr_amd import ops
    B, H, W, C = 2, 32, 32, 64
    g = torch.Generator().manual_seed(7)
    P = lambda *s, k=1.0, o=0.0: torch.nn.Parameter((torch.randn(*s, generator=g) * k + o).cuda())
    x0 = torch.randn(B, H, W, C, generator=g).cuda().to(dtype)
    w1, w2 = P(C, C, 3, 3, k=0.05), P(C, C, 3, 3, k=0.05)
    g1, b1, g2, b2 = P(C, k=0.2, o=1.0), P(C, k=0.1), P(C, k=0.2, o=1.0), P(C, k=0.1)
    wd, gd, bd = (P(C, C, 1, 1, k=0.1), P(C, k=0.2, o=1.0), P(C, k=0.1)) if project else (None, None, None)
    dout = torch.randn(B, H, W, C, generator=g).cuda().to(dtype)
    params = [p for p in (w1, g1, b1, w2, g2, b2, wd, gd, bd) if p is not None]

    def run(flag):
        monkeypatch.setattr(ops, "bn_relu_mask", flag)
        bns = tuple((torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), 0.1, 1e-5, True) for _ in range(3 if project else 2))
        x = x0.clone().requires_grad_()
        out = ops.res_unit(x, w1, g1, b1, w2, g2, b2, wd, gd, bd, 1, 1.0, True, bns)
        grads = torch.autograd.grad(out, [x] + params, dout)
        torch.cuda.synchronize()
        return [out.detach()] + [t.detach().clone() for t in grads]

    on, off = run(True), run(False)
    assert len(on) == len(off) == 2 + len(params)
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), i
