"""GPU: the per-channel kernels (K4/K5, csrc/elementwise.hip) on operands for which their arithmetic is exact, compared
element by element at zero tolerance with the fp64 references of tests/perchannel_exact_ref.py (which also has the
reasons, the preconditions and the per-element bounds of the few cases that cannot be exact: batch statistics over a pixel
count that is no power of two).  Every call states the launches it must make and proves them with the launch census.
What this pins is indexing -- pixels, chunks, lane groups, channel slices, partial rows, the argmax -- and the rounding of
the bf16 stores; dynamic range stays with the norm tests of test_elementwise_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

from tests import perchannel_exact_ref as X

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
K4 = ("bn_stats", "bn_fold_rows", "bn_finalize", "bn_apply", "bn_bwd_reduce", "bn_bwd_finalize", "bn_bwd_apply", "bn_fold",
      "bn_reduce_params", "act_backward", "act_backward_bias", "gate_pool", "gate_pool_finalize", "gate_scale",
      "gate_backward_reduce", "gate_backward_finalize", "gate_backward_apply", "gate_mlp_forward", "gate_mlp_hidden",
      "gate_mlp_out", "gate_mlp_backward", "gate_mlp_bwd_hidden", "gate_mlp_bwd_in", "gate_mlp_wgrad")
OUTSIDE, BESIDE = 7.0, 5.0       # sentinel of a result buffer outside its slice; what lies beside an operand's slice


def _k():
    from jspsr_amd import kernels
    return kernels


def _lib():
    from jspsr_amd import _lib as L
    return L


def _census():
    lib = _lib().load()
    return {n: lib.jspsr_launch_count(n.encode()) for n in K4}


class _Launches:
    """with _Launches(want, tag): ... -- the K4/K5 launches made inside are exactly `want` (name -> count)."""

    def __init__(self, want, tag):
        assert set(want) <= set(K4), want
        self.want, self.tag = {n: want.get(n, 0) for n in K4}, tag

    def __enter__(self):
        self.before = _census()

    def __exit__(self, et, ev, tb):
        if et is None:
            after = _census()
            made = {n: after[n] - self.before[n] for n in K4}
            assert made == self.want, f"{self.tag}: launched { {k: v for k, v in made.items() if v} }, the case names { {k: v for k, v in self.want.items() if v} }"


def act(t, dt):
    return t.float().cuda().to(TORCH_DT[dt]).contiguous()


def par(t):
    return t.float().cuda().contiguous()


def in_slice(t, dt):
    """The operand as channels [32, 32 + C) of a tensor of pitch C + 64 whose other channels hold BESIDE."""
    w = torch.full(tuple(t.shape[:3]) + (t.shape[3] + X.SLICE_PAD,), BESIDE, dtype=TORCH_DT[dt], device="cuda")
    w[..., X.SLICE_OFF:X.SLICE_OFF + t.shape[3]] = act(t, dt)
    return w, w.narrow(3, X.SLICE_OFF, t.shape[3])


def beside_untouched(w, C, value, tag):
    rest = torch.cat((w[..., :X.SLICE_OFF], w[..., X.SLICE_OFF + C:]), 3)
    assert (rest == value).all(), f"{tag}: wrote outside the channel slice"


def can_slice(geo):
    return geo.C in X.SLICE_WIDTHS[geo.dt] and geo.W > 1


def nan_like(shape, dtype):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm forward
# ------------------------------------------------------------------------------------------------------------------

def _forward(c, geo, training, eps, rm, rv, tag, launches, partial=None, stats_only=False, res_affine=None):
    """One bn_forward call on the operands of case c; returns (y (B,H,W,C), mean, invstd, mask or None)."""
    K, dt = _k(), geo.dt
    sliced = c["sliced"] and not stats_only
    xw = resw = None
    if sliced:
        xw, x = in_slice(c["x"], dt)
        resw, res = in_slice(c["res"], dt)
        out = torch.full(tuple(c["shape"][:3]) + (geo.C + X.SLICE_PAD,), OUTSIDE, dtype=TORCH_DT[dt], device="cuda")
    else:
        x, res = act(c["x"], dt), (act(c["res"], dt) if c["with_res"] else None)
        out = None if stats_only else nan_like(c["shape"], TORCH_DT[dt])
    raff = res_affine if res_affine is not None else (par(c["raff"]) if c["with_raff"] else None)
    with _Launches(launches, tag):
        r = K.bn_forward(x, par(c["gamma"]), par(c["beta"]), rm, rv, 0.1, eps, training, relu=c["relu"], res=res,
                         res_scale=c["res_scale"], out=out, out_coff=X.SLICE_OFF if sliced else 0, partial=partial,
                         res_affine=raff, stats_only=stats_only, want_mask=c["want_mask"] and not stats_only)
    y = r[0]
    if sliced:
        beside_untouched(y, geo.C, OUTSIDE, tag)
        beside_untouched(xw, geo.C, BESIDE, tag + " (x)")
        y = y[..., X.SLICE_OFF:X.SLICE_OFF + geo.C]
    return y, r[1], r[2], (r[3] if len(r) > 3 else None)


def run_bn_eval(geo):
    """Eval mode, eps = 0: y, save_mean, save_invstd and the mask bytes bit for bit, every variant; bn_fold, bn_reduce_params
    and stats_only's (scale | shift) on the same parameters; the latter consumed as res_affine."""
    K, dt = _k(), geo.dt
    n = 0
    for variant in X.BN_VARIANTS:
        c = X.bn_eval_case(geo, variant)
        if c["sliced"] and not can_slice(geo):
            continue
        tag = f"{X.geo_id(geo)}/bn_eval/{variant}"
        X.preconditions(c, dt)
        rm, rv = par(c["mean"]), par(c["var"])
        y, mean, invstd, mask = _forward(c, geo, False, 0.0, rm, rv, tag, {"bn_finalize": 1, "bn_apply": 1})
        X.check_exact(y, c["y"], tag, dt)
        X.check_exact(mean, c["save_mean"], tag + ": save_mean")
        X.check_exact(invstd, c["save_invstd"], tag + ": save_invstd")
        assert torch.equal(rm.cpu(), c["mean"].float()) and torch.equal(rv.cpu(), c["var"].float()), f"{tag}: eval mode moved the running statistics"
        if c["want_mask"]:
            assert mask.dtype == torch.uint8 and mask.numel() == c["mask"].numel(), tag
            X.check_exact(mask.reshape(c["npix"], -1), c["mask"].reshape(c["npix"], -1), tag + ": mask bytes [pixel][C / vec]")
        n += 1
    c = X.bn_eval_case(geo, "plain")
    tag = f"{X.geo_id(geo)}/bn_eval"
    with _Launches({"bn_fold": 1}, tag + "/fold"):
        sc, sh = K.bn_fold(par(c["gamma"]), par(c["beta"]), par(c["mean"]), par(c["var"]), 0.0, 0.5)
    X.check_exact(sc, (c["scale"] * 0.5), tag + ": bn_fold scale")
    X.check_exact(sh, (c["shift"] * 0.5), tag + ": bn_fold shift")
    with _Launches({"bn_reduce_params": 1}, tag + "/reduce_params"):
        rp = K.bn_reduce_params(par(c["gamma"]), par(c["beta"]), par(c["mean"]), par(c["invstd"]))
    X.check_exact(rp, c["red_par"], tag + ": bn_reduce_params")
    # stats_only: the (scale | shift) the full call used, and a second BatchNorm consuming it: y = relu(bn(x) / 2 + (x sc + sh))
    aff, mean, invstd, _ = _forward(c, geo, False, 0.0, par(c["mean"]), par(c["var"]), tag + "/stats_only", {"bn_finalize": 1}, stats_only=True)
    X.check_exact(aff, torch.stack((c["scale"], c["shift"])), tag + ": stats_only (scale | shift)")
    X.check_exact(mean, c["save_mean"], tag + ": stats_only save_mean")
    c2 = dict(c, relu=True, with_res=True, res=c["x"], res_scale=0.5)
    y, _, _, _ = _forward(c2, geo, False, 0.0, par(c["mean"]), par(c["var"]), tag + "/res_affine of stats_only",
                          {"bn_finalize": 1, "bn_apply": 1}, res_affine=aff)
    X.check_exact(y, torch.relu(c["pre"] * 0.5 + c["pre"]), tag + ": res_affine of stats_only", dt)
    return n


def run_bn_train(geo, partial=False):
    """Training mode: save_mean bit for bit, save_invstd and the running statistics within 4 fp32 ulps of fp64, y within
    its per-element bound, the mask bytes those of the kernel's own y.  partial: the statistics handed in as rows."""
    dt = geo.dt
    n = 0
    for variant in X.BN_VARIANTS:
        c = X.bn_train_case(geo, variant)
        if c["sliced"] and not can_slice(geo):
            continue
        tag = f"{X.geo_id(geo)}/bn_train/{variant}"
        X.preconditions(c, dt)
        rm, rv = par(c["mean"]), par(c["var"])
        y, mean, invstd, mask = _forward(c, geo, True, 1e-5, rm, rv, tag, {"bn_stats": 1, "bn_finalize": 1, "bn_apply": 1})
        X.check_exact(mean, c["save_mean"], tag + ": save_mean")
        for name, got, ref in (("save_invstd", invstd, c["invstd64"]), ("running_mean", rm, c["rm64"]), ("running_var", rv, c["rv64"])):
            u = X.ulps32(got.cpu(), ref).max().item()
            assert u <= 4, f"{tag}: {name} is {u:.2f} fp32 ulps from fp64"
        X.check_bound(y.float().reshape(c["shape"]), c["y64"], c["bound"], tag)
        if c["want_mask"]:
            assert torch.equal(mask.cpu(), X.mask_bytes(y.float().cpu(), dt)), f"{tag}: mask bytes differ from the bits of the stored y"
        n += 1
        if partial and variant in ("plain", "res_relu_mask"):
            for rows in X.PARTIAL_ROWS:
                rm2, rv2 = par(c["mean"]), par(c["var"])
                t2 = f"{tag}/partial={rows}"
                y2, mean2, invstd2, mask2 = _forward(c, geo, True, 1e-5, rm2, rv2, t2,
                                                     {"bn_fold_rows": int(rows > 256), "bn_finalize": 1, "bn_apply": 1},
                                                     partial=X.partial_rows(c, rows).cuda())
                for name, a, b in (("y", y2, y), ("save_mean", mean2, mean), ("save_invstd", invstd2, invstd), ("running_mean", rm2, rm),
                                   ("running_var", rv2, rv)):
                    assert torch.equal(a, b), f"{t2}: {name} differs from the call that took its own statistics"
                assert mask is None or torch.equal(mask2, mask), t2
                n += 1
    # stats_only in training mode: the same statistics as the full call
    c = X.bn_train_case(geo, "plain")
    tag = f"{X.geo_id(geo)}/bn_train/stats_only"
    rm, rv, rm2, rv2 = par(c["mean"]), par(c["var"]), par(c["mean"]), par(c["var"])
    _, mean, invstd, _ = _forward(c, geo, True, 1e-5, rm, rv, tag, {"bn_stats": 1, "bn_finalize": 1, "bn_apply": 1})
    aff, mean2, invstd2, _ = _forward(c, geo, True, 1e-5, rm2, rv2, tag, {"bn_stats": 1, "bn_finalize": 1}, stats_only=True)
    assert torch.equal(mean, mean2) and torch.equal(invstd, invstd2) and torch.equal(rm, rm2) and torch.equal(rv, rv2), tag
    assert torch.equal(aff[0], par(c["gamma"]) * invstd), tag + ": scale is not gamma * save_invstd"
    return n


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm backward
# ------------------------------------------------------------------------------------------------------------------

def _backward(dy, y, x, gamma, beta, mean, invstd, training, relu, res_scale, want_dres, mask=None, ext_partial=None):
    """jspsr_bn_backward as kernels.bn_backward calls it, but into result buffers pre-filled with NaN: every element of
    dx, dres, dgamma, dbeta must have been written."""
    K, L = _k(), _lib()
    lib = L.load()
    B, H, W, C = x.shape
    dx = nan_like((B, H, W, C), x.dtype)
    dres = nan_like((B, H, W, C), x.dtype) if want_dres else None
    dgamma, dbeta = nan_like((C,), torch.float32), nan_like((C,), torch.float32)
    d = K._dt(x)
    ws = K._workspace(d, C, 1, x.device)
    if mask is not None:
        assert mask.numel() == lib.jspsr_bn_mask_bytes(d, B * H * W, C)
    p = lambda t: t.data_ptr() if t is not None else None
    L.check(lib.jspsr_bn_backward(d, dy.data_ptr(), K.pitch(dy), 0, p(y), K.pitch(y) if y is not None else 0, 0, x.data_ptr(),
                                  K.pitch(x), 0, gamma.data_ptr(), p(beta), mean.data_ptr(), invstd.data_ptr(), int(training),
                                  int(relu), float(res_scale), dx.data_ptr(), p(dres), dgamma.data_ptr(), dbeta.data_ptr(), 0,
                                  B * H * W, C, ws.data_ptr(), p(ext_partial), ext_partial.shape[0] if ext_partial is not None else 0,
                                  p(mask), K._stream()), "jspsr_bn_backward")
    return dx, dres, dgamma, dbeta


def _check_backward(c, got, tag, dt):
    dx, dres, dgamma, dbeta = got
    X.check_exact(dgamma, c["dgamma"], tag + ": dgamma")
    X.check_exact(dbeta, c["dbeta"], tag + ": dbeta")
    if c["want_dres"]:
        X.check_exact(dres, c["dz"], tag + ": dres", dt)
    else:
        assert dres is None
    if c["exact"]:
        X.check_exact(dx, c["dx"], tag + ": dx", dt)
    else:
        assert not torch.isnan(dx.float()).any(), f"{tag}: dx has elements that were not written"
        X.check_bound(dx.float(), c["dx"], c["bound"], tag + ": dx")


def run_bn_backward(geo, extras=False):
    """Modes 0, 1 (from y), 1 (from the bit mask), 2, with and without dres, training 0 and 1: bit for bit wherever the pixel
    count is a power of two or training is off; on ragged counts in training mode dgamma, dbeta, dres bit for bit and dx
    within its bound.  extras: grads_into, ext_partial rows, sliced operands."""
    K, dt = _k(), geo.dt
    n = 0
    for mode in X.BWD_MODES:
        for training in (False, True):
            c = X.bn_bwd_case(geo, mode, training)
            f = c["fwd"]
            tag = f"{X.geo_id(geo)}/bn_bwd/{mode}/training={int(training)}"
            X.preconditions(c, dt)
            dy, x = act(f["dy"], dt), act(f["x"], dt)
            y = act(f["y"], dt) if mode.startswith("1y") else None
            mask = f["mask"].cuda() if mode.startswith("1m") else None
            args = (par(f["gamma"]), par(f["beta"]) if mode == "2" else None, par(f["mean"]), par(f["invstd"]), training, c["relu"],
                    f["res_scale"], c["want_dres"])
            with _Launches({"bn_bwd_reduce": 1, "bn_bwd_finalize": 1, "bn_bwd_apply": 1}, tag):
                got = _backward(dy, y, x, *args, mask=mask)
            _check_backward(c, got, tag, dt)
            n += 1
            if not extras:
                continue
            if mode in ("1y", "1y_dres") and can_slice(geo):
                (dyw, dys), (xw, xs), (yw, ys) = in_slice(f["dy"], dt), in_slice(f["x"], dt), in_slice(f["y"], dt)
                with _Launches({"bn_bwd_reduce": 1, "bn_bwd_finalize": 1, "bn_bwd_apply": 1}, tag + "/slices"):
                    got = _backward(dys, ys, xs, *args)
                _check_backward(c, got, tag + "/slices", dt)
                for w in (dyw, xw, yw):
                    beside_untouched(w, geo.C, BESIDE, tag + "/slices")
                n += 1
            if mode == "1y_dres" and not training:       # the wrapper's grads_into: added to integers already there
                acc = par(f["acc0"])
                with _Launches({"bn_bwd_reduce": 1, "bn_bwd_finalize": 1, "bn_bwd_apply": 1}, tag + "/grads_into"):
                    dx, dres, g0, g1 = K.bn_backward(dy, y, x, par(f["gamma"]), par(f["mean"]), par(f["invstd"]), training, 1, f["res_scale"],
                                                     want_dres=True, grads_into=(acc[0], acc[1]))
                assert g0 is None and g1 is None
                X.check_exact(acc[0], f["acc0"][0] + c["dgamma"], tag + "/grads_into: dgamma")
                X.check_exact(acc[1], f["acc0"][1] + c["dbeta"], tag + "/grads_into: dbeta")
                X.check_exact(dx, c["dx"], tag + "/grads_into: dx", dt)
                n += 1
            if mode == "2" and c["exact"] and geo.C <= 520:      # (1500 rows of 2 x 520 floats at most)
                for rows in X.EXT_ROWS:
                    t2 = f"{tag}/ext_partial={rows}"
                    with _Launches({"bn_fold_rows": int(rows > 1024), "bn_bwd_finalize": 1, "bn_bwd_apply": 1}, t2):
                        got = _backward(dy, None, x, *args, ext_partial=X.partial_rows(c, rows, 0.25).cuda())
                    _check_backward(c, got, t2, dt)
                    n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------
# ReLU / bias backward
# ------------------------------------------------------------------------------------------------------------------

def run_act(geo):
    K, dt = _k(), geo.dt
    n = 0
    for relu in (True, False):
        c = X.act_case(geo, relu)
        tag = f"{X.geo_id(geo)}/act_backward/relu={int(relu)}"
        X.preconditions(c, dt)
        dy, y = act(c["dy"], dt), (act(c["y"], dt) if relu else None)
        forms = [("plain", dy, y, {}), ("no_dz", dy, y, {"want_dz": False}), ("no_dbias", dy, y, {"want_dbias": False}),
                 ("dz_wide", dy, y, {"dz_channels": geo.C + 2 * X.VEC[dt]})]
        if geo.W > 1:
            forms.append(("slices", in_slice(c["dy"], dt)[1], in_slice(c["y"], dt)[1] if relu else None, {}))
        for form, a, b, kw in forms:
            with _Launches({"act_backward": 1, "act_backward_bias": int(kw.get("want_dbias", True))}, f"{tag}/{form}"):
                dz, dbias = K.act_backward(a, b, relu, **kw)
            if kw.get("want_dz", True):
                X.check_exact(dz[..., :geo.C], c["dz"], f"{tag}/{form}: dz", dt)
                assert (dz[..., geo.C:] == 0).all(), f"{tag}/{form}: the channel padding of dz is not zero"
            else:
                assert dz is None
            if kw.get("want_dbias", True):
                X.check_exact(dbias, c["dbias"], f"{tag}/{form}: dbias")
            else:
                assert dbias is None
            n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------
# channel gate
# ------------------------------------------------------------------------------------------------------------------

def run_gate(geo):
    K, dt = _k(), geo.dt
    cases = [(form, None) for form in X.GATE_FORMS if not (form == "ties" and geo.H * geo.W < 4)]
    if (geo.H, geo.W) == (5, 7):
        cases.append(("ties", 3))
    n = 0
    for form, B in cases:
        c = X.gate_case(geo, form, B)
        tag = f"{X.geo_id(geo)}/gate/{form}/B={c['B']}"
        X.preconditions(c, dt)
        sh = (c["B"], geo.H, geo.W, geo.C)
        x, dy = act(c["x"].reshape(sh), dt), act(c["dy"].reshape(sh), dt)
        with _Launches({"gate_pool": 1, "gate_pool_finalize": 1}, tag + "/pool"):
            avg, mx, amax = K.gate_pool(x)
        X.check_exact(mx, c["mx"], tag + ": mx")
        assert amax.dtype == torch.int32
        X.check_exact(amax, c["amax"], tag + ": amax (the smallest pixel index of the maximum)")
        X.check_exact(avg, c["avg"], tag + ": avg")
        s = par(c["s"])
        with _Launches({"gate_scale": 1}, tag + "/scale"):
            y = K.gate_scale(x, s)
        X.check_exact(y.reshape(c["B"], c["npix"], geo.C), c["scaled"], tag + ": gate_scale", dt)
        with _Launches({"gate_backward_reduce": 1, "gate_backward_finalize": 1}, tag + "/reduce"):
            ds = K.gate_backward_reduce(dy, x)
        X.check_exact(ds, c["ds"], tag + ": gate_backward_reduce")
        am = c["amax"].cuda()
        for name, davg in (("davg", c["davg"]), ("davg=0", torch.zeros_like(c["davg"]))):
            r = X.gate_apply_ref(c, dt, davg)
            with _Launches({"gate_backward_apply": 1}, f"{tag}/apply/{name}"):
                dx = K.gate_backward_apply(dy, s, par(davg), par(c["dmax"]), am).reshape(c["B"], c["npix"], geo.C)
            if r["exact"]:
                X.check_exact(dx, r["dx"], f"{tag}: gate_backward_apply/{name}", dt)
            else:
                X.check_bound(dx.float(), r["dx"], r["bound"], f"{tag}: gate_backward_apply/{name}")
        # the dmax term alone: exactly one pixel per (image, channel), the argmax
        dx = K.gate_backward_apply(torch.zeros_like(dy), s, par(torch.zeros_like(c["davg"])), par(c["dmax"]), am)
        dx = dx.float().reshape(c["B"], c["npix"], geo.C).cpu()
        assert ((dx != 0).sum(1) == 1).all(), f"{tag}: the dmax term landed on {(dx != 0).sum(1).unique().tolist()} pixels per (image, channel)"
        assert torch.equal(dx.double(), c["hit"] * c["dmax"].unsqueeze(1)), f"{tag}: the dmax term is not at the argmax"
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------
_WIDTHS = [(dt, C) for dt in ("f32", "bf16") for C in X.CHANNELS[dt]]
_WIDTH_IDS = [f"{dt}-c{C}" for dt, C in _WIDTHS]


def _geos(dt, C):
    return [g for g in X.GEOS if g.dt == dt and g.C == C]


@pytest.mark.parametrize("dt,C", _WIDTHS, ids=_WIDTH_IDS)
def test_bn_forward_eval_exact(dt, C):
    """Plain, ReLU, residual with res_scale, residual + ReLU + mask, res_affine, out= a slice; bn_fold, bn_reduce_params,
    stats_only and its consumption as res_affine: every raster of the width, bit for bit."""
    for geo in _geos(dt, C):
        run_bn_eval(geo)


@pytest.mark.parametrize("dt,C", _WIDTHS, ids=_WIDTH_IDS)
def test_bn_forward_training(dt, C):
    """Batch statistics: save_mean exact, 4 ulps on save_invstd and the running statistics, per-element bound on y; partial=
    rows (copied up to 256, folded above, never a statistics pass) give the bits of the call that made its own -- on one
    ragged and one power-of-two raster, the rows feeding only the per-channel finalize."""
    for geo in _geos(dt, C):
        run_bn_train(geo, partial=(geo.B, geo.H, geo.W) in (X.R35, X.R256))


@pytest.mark.parametrize("dt,C", _WIDTHS, ids=_WIDTH_IDS)
def test_bn_backward_exact(dt, C):
    """Every mask mode (bf16 mode 2 among them), with and without dres, training off and on, grads_into, ext_partial rows
    (read in place up to 1024, folded above, never a reduce pass), sliced dy / x / y."""
    for geo in _geos(dt, C):
        run_bn_backward(geo, extras=True)


@pytest.mark.parametrize("dt,C", _WIDTHS, ids=_WIDTH_IDS)
def test_act_backward_exact(dt, C):
    """dz and dbias bit for bit: ReLU on / off, without dz, without dbias, a padded dz pitch, y and dy as slices."""
    for geo in _geos(dt, C):
        run_act(geo)


@pytest.mark.parametrize("dt,C", _WIDTHS, ids=_WIDTH_IDS)
def test_channel_gate_exact(dt, C):
    """gate_pool (sum, maximum, first maximal pixel: ties across sub-lanes, rows and chunks, pixel 0 and the last one, an
    all-negative image, B = 3), gate_scale, gate_backward_reduce, gate_backward_apply."""
    for geo in _geos(dt, C):
        run_gate(geo)


@pytest.mark.parametrize("shape", X.MLP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gate_mlp_exact(shape):
    """The chip-wide and the one-workgroup-per-image kernels on integer operands: hid and every gradient bit for bit against
    fp64 (Ch above 128: several slabs of w2, a ragged last one), the forward's s within 4 * 2^-24 of fp64 per element."""
    K = _k()
    c = X.mlp_case(*shape)
    X.preconditions(c, "f32")
    B, C, Ch = shape
    avg, mx, w1, w2, ds = (par(c[k]) for k in ("avg", "mx", "w1", "w2", "ds"))
    prev = K.gate_mlp_legacy()
    try:
        for legacy in (0, 1):
            K.gate_mlp_legacy(legacy)
            tag = f"gate_mlp {shape} legacy={legacy}"
            fwd = {"gate_mlp_forward": 1} if legacy else {"gate_mlp_hidden": 1, "gate_mlp_out": 1}
            bwd = {"gate_mlp_backward": 1, "gate_mlp_wgrad": 1} if legacy else {"gate_mlp_bwd_hidden": 1, "gate_mlp_bwd_in": 1, "gate_mlp_wgrad": 1}
            with _Launches(fwd, tag):
                s, hid = K.gate_mlp_forward(avg, mx, w1, w2)
            X.check_exact(hid, c["hid"], tag + ": hid")
            err = (s.cpu().double() - c["s"]).abs().max().item()
            print(f"{tag}: max |s - fp64| = {err:.3e} (limit {X.MLP_S_LIMIT:.3e})")
            assert err <= X.MLP_S_LIMIT, f"{tag}: s is {err:.3e} from fp64"
            with _Launches(bwd, tag):
                got = K.gate_mlp_backward(ds, par(c["s_in"]), par(c["hid"]), avg, mx, w1, w2)
            for name, g in zip(("davg", "dmax", "dw1", "dw2"), got):
                X.check_exact(g, c[name], f"{tag}: {name}")
    finally:
        K.gate_mlp_legacy(int(prev))


@pytest.mark.parametrize("dt,C", [("f32", 1792), ("bf16", 3584)])
def test_workspace_contract_of_the_forward_with_external_rows(dt, C):
    """jspsr_bn_forward with 300 external statistics rows at 7 channel blocks, through the C ABI with a workspace of exactly
    the bytes promised plus a 2 MiB tail of a byte pattern: asserted BEFORE the launch that everything the call may write
    (scale | shift, then 256 folded rows: 514 C floats) lies inside that one allocation, after it that the tail is untouched
    and the statistics are right."""
    K, L = _k(), _lib()
    lib = L.load()
    geo = X.Geo(dt, C, 1, 4, 4)
    c = X.bn_train_case(geo, "plain")
    rows, tail = 300, 2 << 20
    promised = lib.jspsr_reduce_workspace_bytes(K.F32 if dt == "f32" else K.BF16, C, 1)
    assert promised == X.promised_floats(dt, C, 1) * 4 + 64
    ws = torch.empty(promised + tail, dtype=torch.uint8, device="cuda")
    ws[promised:] = 0xA5
    writes = X.written_floats("bn_forward", dt, C, 1, 16, ext_rows=rows) * 4
    assert writes <= ws.numel(), "the call would leave the allocation: not launched"
    assert writes <= promised, f"bn_forward(ext_partial of {rows} rows) writes {writes} bytes, {promised} are promised"
    x, y = act(c["x"], dt), nan_like(c["shape"], TORCH_DT[dt])
    p = X.partial_rows(c, rows).cuda()
    mean, invstd = nan_like((C,), torch.float32), nan_like((C,), torch.float32)
    gamma, beta = par(c["gamma"]), par(c["beta"])
    with _Launches({"bn_fold_rows": 1, "bn_finalize": 1, "bn_apply": 1}, f"workspace {dt} {C}"):
        L.check(lib.jspsr_bn_forward(K._dt(x), x.data_ptr(), C, 0, None, 0, 0, y.data_ptr(), C, 0, gamma.data_ptr(), beta.data_ptr(),
                                     None, None, 0.1, 1e-5, 1, 0, 1.0, mean.data_ptr(), invstd.data_ptr(), 16, C, p.data_ptr(), rows,
                                     None, None, None, ws.data_ptr(), K._stream()), "jspsr_bn_forward")
    torch.cuda.synchronize()
    assert (ws[promised:] == 0xA5).all(), "the call wrote past the bytes jspsr_reduce_workspace_bytes promises"
    X.check_exact(mean, c["save_mean"], "save_mean")
    X.check_bound(y.float(), c["y64"], c["bound"], f"workspace {dt} {C}: y")


def run_table(name):
    """Child-process entry: every operator on every geometry of CHILD_TABLES[name]."""
    _, geos = X.CHILD_TABLES[name]
    n = 0
    for geo in geos:
        run_bn_eval(geo)
        run_bn_train(geo, partial=False)
        run_bn_backward(geo, extras=False)
        run_act(geo)
        run_gate(geo)
        n += 1
    torch.cuda.synchronize()
    print(f"exact ok: {name}, {n} cases")


@pytest.mark.parametrize("name", sorted(X.CHILD_TABLES))
def test_switched_geometry_exact_in_a_child_process(name):
    """The library reads JSPSR_RED_BLOCKS once per process: with 2 blocks a 50 x 50 raster is two chunks of 1250 pixels, and
    the four-pixels-in-flight main loop runs at the narrow widths (1, 3, 5, 16 / 8 lane groups, up to 64 pixels side by side
    in a row of lanes), where under the default target only the tail loop ever does."""
    env, geos = X.CHILD_TABLES[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"from tests.test_perchannel_exact_gpu import run_table; run_table({name!r})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and f"exact ok: {name}, {len(geos)} cases" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
