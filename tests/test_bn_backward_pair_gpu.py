"""GPU: the two BatchNorm backwards of a projecting residual block in one reduce and one apply pass (jspsr_bn_backward_pair).

The block's second BatchNorm (residual + ReLU, bit mask) and its shortcut's BatchNorm take the same masked gradient; the pair
call never writes it.  The yardstick is the two separate calls -- bn_backward(..., want_dres=True, mask=...) and then
bn_backward(dres, ..., relu=0) -- and the check is torch.equal on dz2, dzd, both dgamma and both dbeta, over every option:
dy dense or a channel slice of a wider tensor, res_scale 1.0 and 0.5, each layer's training flag, gradients returned or added
to pre-filled buffers.  An fp64 torch restatement of the same formulas bounds the results themselves, under the tolerance of
test_bn_backward_mask_gpu.py (relative norm, 1e-5 fp32 / 1.5e-2 bf16).

Shapes.  Per lane the reduce pass walks a chunk's pixels four per trip, then one by one (the apply pass one by one
throughout); a chunk has at least 64 pixels and a tensor at most 1024 / ceil(C / vec / 64) chunks.  1x5x7 is one chunk walked by the tail loop alone; 2x33x17 makes 18 chunks of 63 with a
ragged last one of 51; 2x96x100 makes 300 chunks.  At C / vec < 64 several pixels share a 64-lane row and these rasters
never fill a four-pixel trip, so two more cases do: 64 lanes per pixel (bf16 C = 512, fp32 C = 256) on 2x33x17 -- three full
trips and a tail of up to three pixels per lane -- and the flagship's 64 bf16 channels on 1x368x360, 1020 chunks of 130 with
a ragged last one.  More than 1024 partial rows cannot be produced: make_red caps the chunk count at JSPSR_RED_BLOCKS (1024
by default, read once per process), at any size."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

RASTERS = [(1, 5, 7), (2, 33, 17), (2, 96, 100)]
WIDTHS = [(torch.bfloat16, 8), (torch.bfloat16, 64), (torch.bfloat16, 72), (torch.float32, 4), (torch.float32, 12)]
CASES = [(dt, C) + r for dt, C in WIDTHS for r in RASTERS] + \
        [(torch.bfloat16, 512, 2, 33, 17), (torch.float32, 256, 2, 33, 17), (torch.bfloat16, 64, 1, 368, 360)]
PARAMS = [pytest.param(*c, id=f"{str(c[0])[6:]}-C{c[1]}-{'x'.join(map(str, c[2:]))}") for c in CASES]
NAMES = ("dz2", "dzd", "dgamma2", "dbeta2", "dgammad", "dbetad")
PAIR_LABELS = ("bn_bwd_reduce_pair", "bn_bwd_finalize_pair", "bn_bwd_apply_pair")
SOLO_LABELS = ("bn_bwd_reduce", "bn_bwd_finalize", "bn_bwd_apply")


def _k():
    from jspsr_amd import kernels
    return kernels


def _census(labels=PAIR_LABELS + SOLO_LABELS):
    from jspsr_amd import _lib
    lib = _lib.load()
    return {n: lib.jspsr_launch_count(n.encode()) for n in labels}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def _operands(dtype, C, B, H, W):
    """z2, zd, dy (dense and as a channel slice), parameters, saved statistics and the forward's own bit mask."""
    K = _k()
    vec = K.epc(dtype)
    g = torch.Generator().manual_seed(100 * C + 10 * H + W)
    rnd = lambda *s: torch.randn(*s, generator=g)
    z2 = (rnd(B, H, W, C) * 1.7 + 0.4).cuda().to(dtype)
    zd = (rnd(B, H, W, C) * 0.8 - 0.3).cuda().to(dtype)
    dy = rnd(B, H, W, C).cuda().to(dtype)
    wide = torch.full((B, H, W, C + 2 * vec), float("nan"), dtype=dtype, device="cuda")
    wide[..., vec:vec + C] = dy
    g2, b2, gd, bd = (1 + 0.2 * rnd(C)).cuda(), (0.1 * rnd(C)).cuda(), (1 + 0.2 * rnd(C)).cuda(), (0.1 * rnd(C)).cuda()
    fill = [(rnd(C) * 3).cuda() for _ in range(4)]                      # what the accumulating form adds to
    out = {}
    for rs in (1.0, 0.5):
        # the block's forward: the shortcut's BatchNorm as statistics + affine, applied inside bn2's pass
        affd, md, idd = K.bn_forward(zd, gd, bd, None, None, 0.1, 1e-5, True, False, stats_only=True)
        y, m2, i2, mask = K.bn_forward(z2, g2, b2, None, None, 0.1, 1e-5, True, True, zd, rs, res_affine=affd, want_mask=True)
        out[rs] = dict(y=y, m2=m2, i2=i2, md=md, idd=idd, mask=mask)
    torch.cuda.synchronize()
    return dict(z2=z2, zd=zd, dy=dy, dy_slice=wide[..., vec:vec + C], g2=g2, gd=gd, fill=fill, fwd=out)


def _two_calls(K, o, f, dy, rs, tr2, trd, acc):
    s2, sd = ((o["fill"][0].clone(), o["fill"][1].clone()), (o["fill"][2].clone(), o["fill"][3].clone())) if acc else (None, None)
    dz2, dres, dg2, db2 = K.bn_backward(dy, None, o["z2"], o["g2"], f["m2"], f["i2"], tr2, 1, rs, want_dres=True, mask=f["mask"],
                                        grads_into=s2)
    dzd, _, dgd, dbd = K.bn_backward(dres, None, o["zd"], o["gd"], f["md"], f["idd"], trd, 0, 1.0, grads_into=sd)
    return (dz2, dzd) + ((s2 + sd) if acc else (dg2, db2, dgd, dbd))


def _pair(K, o, f, dy, rs, tr2, trd, acc):
    s2, sd = ((o["fill"][0].clone(), o["fill"][1].clone()), (o["fill"][2].clone(), o["fill"][3].clone())) if acc else (None, None)
    r = K.bn_backward_pair(dy, f["mask"], o["z2"], o["g2"], f["m2"], f["i2"], tr2, rs, o["zd"], o["gd"], f["md"], f["idd"], trd,
                           grads_into2=s2, grads_intod=sd)
    if acc:
        assert r[2:] == (None, None, None, None)
    return r[:2] + ((s2 + sd) if acc else r[2:])


@pytest.mark.parametrize("dtype,C,B,H,W", PARAMS)
def test_pair_call_gives_the_bits_of_the_two_calls(dtype, C, B, H, W):
    K = _k()
    o = _operands(dtype, C, B, H, W)
    assert o["dy_slice"].stride(2) > C and not o["dy_slice"].is_contiguous()
    n0 = _census()
    for sl, rs, tr2, trd, acc in itertools.product((False, True), (1.0, 0.5), (True, False), (True, False), (False, True)):
        f = o["fwd"][rs]
        dy = o["dy_slice"] if sl else o["dy"]
        want = _two_calls(K, o, f, dy, rs, tr2, trd, acc)
        got = _pair(K, o, f, dy, rs, tr2, trd, acc)
        for name, a, b in zip(NAMES, got, want):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (name, sl, rs, tr2, trd, acc)
    n1 = _census()
    for n in PAIR_LABELS:        # 32 pair calls, one launch of each kind; the two calls are two of each of theirs
        assert n1[n] - n0[n] == 32, (n, n0, n1)
    for n in SOLO_LABELS:
        assert n1[n] - n0[n] == 64, (n, n0, n1)


@pytest.mark.parametrize("dtype,C,B,H,W", PARAMS)
def test_pair_call_matches_fp64(dtype, C, B, H, W):
    K = _k()
    o = _operands(dtype, C, B, H, W)
    gtol = 1e-5 if dtype == torch.float32 else 1.5e-2          # test_bn_backward_mask_gpu's, for this call
    n = B * H * W
    D = lambda t: t.double().reshape(n, C)
    for rs, tr2, trd in itertools.product((1.0, 0.5), (True, False), (True, False)):
        f = o["fwd"][rs]
        got = _pair(K, o, f, o["dy"], rs, tr2, trd, False)
        dz = torch.where(D(f["y"]) > 0, D(o["dy"]), torch.zeros((), dtype=torch.float64, device="cuda"))
        for x, gam, mean, invstd, tr, scale, names in ((o["z2"], o["g2"], f["m2"], f["i2"], tr2, rs, ("dz2", "dgamma2", "dbeta2")),
                                                       (o["zd"], o["gd"], f["md"], f["idd"], trd, 1.0, ("dzd", "dgammad", "dbetad"))):
            xhat = (D(x) - mean.double()) * invstd.double()
            s, sx = dz.sum(0), (dz * xhat).sum(0)
            a, b = (s / n, sx / n) if tr else (torch.zeros_like(s), torch.zeros_like(s))
            ref = dict(zip(names, ((gam.double() * invstd.double() * scale * (dz - a - xhat * b)).reshape(B, H, W, C), sx * scale, s * scale)))
            for name in names:
                err = _rel(got[NAMES.index(name)], ref[name])
                print(f"rs {rs} training {tr2}/{trd} {name}: rel err {err:.3e} (bound {gtol:g})")
                assert err < gtol, (name, rs, tr2, trd, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride", [1, 2])
def test_res_unit_projection_gradients_do_not_depend_on_the_switch(dtype, stride, monkeypatch):
    from jspsr_amd import ops
    B, H, W, C = 2, 32, 32, 64
    g = torch.Generator().manual_seed(11 + stride)
    P = lambda *s, k=1.0, o=0.0: torch.nn.Parameter((torch.randn(*s, generator=g) * k + o).cuda())
    x0 = torch.randn(B, H, W, C, generator=g).cuda().to(dtype)
    w1, w2, wd = P(C, C, 3, 3, k=0.05), P(C, C, 3, 3, k=0.05), P(C, C, 1, 1, k=0.1)
    g1, b1, g2, b2, gd, bd = P(C, k=0.2, o=1.0), P(C, k=0.1), P(C, k=0.2, o=1.0), P(C, k=0.1), P(C, k=0.2, o=1.0), P(C, k=0.1)
    dout = torch.randn(B, H // stride, W // stride, C, generator=g).cuda().to(dtype)
    params = [w1, g1, b1, w2, g2, b2, wd, gd, bd]

    def run(flag):
        monkeypatch.setattr(ops, "bn_shortcut_merge", flag)
        bns = tuple((torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), 0.1, 1e-5, True) for _ in range(3))
        x = x0.clone().requires_grad_()
        out = ops.res_unit(x, w1, g1, b1, w2, g2, b2, wd, gd, bd, stride, 0.5, True, bns)
        n0 = _census()
        grads = torch.autograd.grad(out, [x] + params, dout)
        torch.cuda.synchronize()
        n1 = _census()
        return [out.detach()] + [t.detach().clone() for t in grads], {k: n1[k] - n0[k] for k in n0}

    assert ops.bn_relu_mask, "the merged backward needs the bit mask (JSPSR_BN_RELU_MASK)"
    (on, n_on), (off, n_off) = run(True), run(False)
    assert len(on) == len(off) == 2 + len(params)
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), i
    # census: merged, the block's backward makes one pair call and no reduce / apply pass for the shortcut layer -- what is
    # left of the plain labels is bn1's (its reduce may ride in conv2's data gradient); apart, bn2 and the shortcut add two
    for n in PAIR_LABELS:
        assert n_on[n] == 1 and n_off[n] == 0, (n, n_on, n_off)
    assert n_on["bn_bwd_apply"] == 1 and n_on["bn_bwd_finalize"] == 1 and n_on["bn_bwd_reduce"] in (0, 1), n_on
    for n in SOLO_LABELS:
        assert n_off[n] == n_on[n] + 2, (n, n_on, n_off)


def test_identity_block_and_mask_switch_keep_the_two_call_path(monkeypatch):
    from jspsr_amd import ops
    B, H, W, C = 1, 16, 16, 64
    g = torch.Generator().manual_seed(3)
    P = lambda *s, k=1.0, o=0.0: torch.nn.Parameter((torch.randn(*s, generator=g) * k + o).cuda())
    w1, w2, wd = P(C, C, 3, 3, k=0.05), P(C, C, 3, 3, k=0.05), P(C, C, 1, 1, k=0.1)
    g1, b1, g2, b2, gd, bd = P(C, k=0.2, o=1.0), P(C, k=0.1), P(C, k=0.2, o=1.0), P(C, k=0.1), P(C, k=0.2, o=1.0), P(C, k=0.1)
    x0 = torch.randn(B, H, W, C, generator=g).cuda()

    def pair_launches(project, mask):
        monkeypatch.setattr(ops, "bn_relu_mask", mask)
        bns = tuple((torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), 0.1, 1e-5, True) for _ in range(3 if project else 2))
        x = x0.clone().requires_grad_()
        out = ops.res_unit(x, w1, g1, b1, w2, g2, b2, *((wd, gd, bd) if project else (None, None, None)), 1, 1.0, True, bns)
        n0 = _census(PAIR_LABELS)
        out.sum().backward()
        torch.cuda.synchronize()
        n1 = _census(PAIR_LABELS)
        return sum(n1[k] - n0[k] for k in n0)

    assert ops.bn_shortcut_merge
    assert pair_launches(True, True) == 3 and pair_launches(False, True) == 0 and pair_launches(True, False) == 0


def test_pair_arguments_are_refused_with_a_code():
    """Each bad call returns JSPSR_EINVAL / JSPSR_EALIGN before any launch; the process lives and the next good call runs."""
    from jspsr_amd import _lib
    K = _k()
    lib = _lib.load()
    o = _operands(torch.bfloat16, 64, 1, 5, 7)
    f = o["fwd"][1.0]
    C, npix = 64, 35
    dx2, dxd = torch.empty_like(o["z2"]), torch.empty_like(o["z2"])
    pg = [torch.empty(C, device="cuda") for _ in range(4)]
    ws = torch.empty(lib.jspsr_bn_backward_pair_workspace_bytes(K.BF16, C), dtype=torch.uint8, device="cuda")
    good = dict(dtype=K.BF16, dy=o["dy"].data_ptr(), dy_cs=C, dy_coff=0, mask=f["mask"].data_ptr(), x2=o["z2"].data_ptr(), x2_cs=C,
                x2_coff=0, gamma2=o["g2"].data_ptr(), mean2=f["m2"].data_ptr(), invstd2=f["i2"].data_ptr(), training2=1,
                res_scale=1.0, xd=o["zd"].data_ptr(), xd_cs=C, xd_coff=0, gammad=o["gd"].data_ptr(),
                meand=f["md"].data_ptr(), invstdd=f["idd"].data_ptr(), trainingd=1, dx2=dx2.data_ptr(), dxd=dxd.data_ptr(),
                dgamma2=pg[0].data_ptr(), dbeta2=pg[1].data_ptr(), accumulate2=0, dgammad=pg[2].data_ptr(), dbetad=pg[3].data_ptr(),
                accumulated=0, npix=npix, C=C, workspace=ws.data_ptr(), stream=K._stream())
    assert len(good) == len(_lib.SIGNATURES["jspsr_bn_backward_pair"][1])
    call = lambda **kw: lib.jspsr_bn_backward_pair(*{**good, **kw}.values())
    n0 = _census(PAIR_LABELS)
    EINVAL, EALIGN = -1, -2
    for kw in (dict(dy=None), dict(mask=None), dict(x2=None), dict(xd=None), dict(dx2=None), dict(dxd=None), dict(gamma2=None),
               dict(invstdd=None), dict(dgammad=None), dict(dbeta2=None), dict(workspace=None), dict(npix=0), dict(dtype=2),
               dict(C=60), dict(C=0), dict(dy_cs=C + 4), dict(dy_coff=4), dict(x2_cs=C + 2), dict(xd_coff=3),
               dict(dy_coff=8), dict(x2_cs=C - 8), dict(xd_coff=-8), dict(dxd=good["dx2"]), dict(dgammad=good["dgamma2"])):
        assert call(**kw) == EINVAL, kw
        assert b"bn_backward_pair" in lib.jspsr_last_error(), kw
    for kw in (dict(dy=good["dy"] + 2), dict(x2=good["x2"] + 8), dict(xd=good["xd"] + 4), dict(dx2=good["dx2"] + 2),
               dict(dxd=good["dxd"] + 8), dict(workspace=good["workspace"] + 4)):
        assert call(**kw) == EALIGN, kw
    assert lib.jspsr_bn_backward_pair_workspace_bytes(K.BF16, 0) == 0
    assert _census(PAIR_LABELS) == n0          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    want = _two_calls(K, o, f, o["dy"], 1.0, True, True, False)
    for a, b in zip((dx2, dxd) + tuple(pg), want):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):          # a mask of another shape
        K.bn_backward_pair(o["dy"], f["mask"][:-1], o["z2"], o["g2"], f["m2"], f["i2"], True, 1.0, o["zd"], o["gd"], f["md"], f["idd"], True)
    with pytest.raises(ValueError):          # operands that disagree
        K.bn_backward_pair(o["dy"], f["mask"], o["z2"], o["g2"], f["m2"], f["i2"], True, 1.0, o["zd"][..., :32], o["gd"], f["md"], f["idd"], True)
