"""GPU: every convolution kernel (conv.hip, conv64.hip, conv128.hip, wgrad.hip) on integer operands, compared element by
element with torch's CPU convolution at zero tolerance (tests/conv_exact_ref.py has the operands, the reference and the
reasons the arithmetic is exact).  Every case names the kernel its launch must take and proves it with the launch census
(jspsr_launch_count) before and after: a case that lands on another kernel fails.  What this pins is indexing -- taps,
pixels, channels, tiles, statistics rows, slices; rounding and dynamic range stay with the norm tests of test_conv_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

from tests import conv_exact_ref as X

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _k():
    from jspsr_amd import kernels
    return kernels


def _census(names):
    from jspsr_amd import _lib
    lib = _lib.load()
    return {n: lib.jspsr_launch_count(n.encode()) for n in names}


class _Launches:
    """with _Launches(names, want, tag): ... -- the launches made inside are exactly `want` (name -> count)."""

    def __init__(self, names, want, tag):
        self.names, self.want, self.tag = names, {n: want.get(n, 0) for n in names}, tag

    def __enter__(self):
        self.before = _census(self.names)

    def __exit__(self, et, ev, tb):
        if et is None:
            after = _census(self.names)
            made = {n: after[n] - self.before[n] for n in self.names}
            assert made == self.want, f"{self.tag}: launched {made}, the case names {self.want}"


def _packed(w, mode, c_pad, dt, tag):
    """jspsr_pack_weight, checked exactly: a packing error is not to be reported as a convolution error."""
    wp = _k().pack_weight(w.cuda(), mode, c_pad, TORCH_DT[dt])
    X.assert_exact(wp.float(), X.pack_ref(w, mode, c_pad), f"{tag}: pack_weight mode {mode}", axes=X.PACK_AXES, hists=X.PACK_HISTS)
    return wp


def run_forward(r, dt, forms):
    K, tdt = _k(), TORCH_DT[dt]
    for form in forms:
        c = X.forward_case(r, form)
        tag = f"{r.name}/{dt}/fwd/{form}"
        wp = _packed(c["w"], 0, r.Cin, dt, tag)
        dev = lambda t: None if t is None else t.cuda()
        x = c["x"].cuda().to(tdt)
        addend = None if c["addend"] is None else c["addend"].cuda().to(tdt)
        out = None
        if form == "slices":
            out = torch.full(tuple(c["want"].shape[:3]) + (c["out_pitch"],), 7.0, dtype=tdt, device="cuda")
        with _Launches(X.CONV_KERNELS, r.fwd, tag):
            y = K.conv2d_forward(x, wp, dev(c["bias"]), r.stride, r.pad, relu=c["relu"], out=out, out_coff=c["out_coff"],
                                 cin=r.Cin, in_coff=c["in_coff"], stats=c["stats"] is not None, scale=dev(c["scale"]),
                                 addend=addend, in_affine=dev(c["in_affine"]), in_relu=c["in_affine"] is not None)
        if c["stats"] is not None:
            y, st = y
            B, oh, ow = c["want"].shape[:3]
            X.assert_exact(X.stats_view(st, B, oh, ow), X.stats_view(c["stats"], B, oh, ow), f"{tag}: statistics rows",
                           axes=X.STATS_AXES, hists=X.STATS_HISTS)
            if c["stats_pairs"]:      # not only the kernel's own numbering: each 16x16 tile's two rows add up to its direct sums
                X.assert_exact(X.fold_rows16(st.cpu(), B, oh, ow).flatten(0, 1), c["stats16"].flatten(0, 1),
                               f"{tag}: statistics per 16x16 tile", axes=X.STATS_AXES, hists=X.STATS_HISTS)
        if form == "slices":
            o = c["out_coff"]
            X.assert_exact(y[..., o:o + r.Cout].float(), c["want"], tag)
            rest = torch.cat((y[..., :o], y[..., o + r.Cout:]), 3)
            assert (rest == 7.0).all(), f"{tag}: wrote outside the channel slice"
        else:
            X.assert_exact(y.float(), c["want"], tag)


def run_dgrad(r, dt, forms):
    K, tdt = _k(), TORCH_DT[dt]
    for form in forms:
        c = X.dgrad_case(r, form)
        tag = f"{r.name}/{dt}/dgrad/{form}"
        wpt = _packed(c["w"], 1, r.Cin, dt, tag)            # conv weight (O = Cin of the row, I = Cout of the row)
        g = c["g"].cuda().to(tdt)
        addend = None if c["addend"] is None else c["addend"].cuda().to(tdt)
        out = torch.full((r.B, r.H, r.W, r.Cout), 7.0, dtype=tdt, device="cuda")      # pixels no tap reaches must be WRITTEN as zeros
        with _Launches(X.CONV_KERNELS, r.dgrad, tag):
            dx = K.conv2d_dgrad(g, wpt, (r.H, r.W), r.stride, r.pad, relu=c["relu"], addend=addend, out=out)
        X.assert_exact(dx.float(), c["want"], tag)


def run_wgrad(r, dt):
    K, tdt = _k(), TORCH_DT[dt]
    for form in r.forms:
        c = X.wgrad_case(r, form, dt)
        tag = f"{r.name}/{dt}/wgrad/{form}"
        G, Xt = c["G"].cuda().to(tdt), c["X"].cuda().to(tdt)
        kw = {}
        if form == "slices":
            Gw, Xw = G, Xt
            G, Xt = G.narrow(3, c["g_coff"], c["cg"]), Xt.narrow(3, c["x_coff"], r.Cin)
        if form == "accumulate":
            kw = {"out": c["init"].cuda().clone(), "accumulate": True}
        if form == "x_affine_relu":
            oh, ow = X.out_hw(r)
            from jspsr_amd import _lib
            assert _lib.load().jspsr_conv2d_wgrad_x_affine_ok(K._dt(G), r.B, oh, ow, c["cg"], r.Cin, 3, 3, 1, 1), tag
            kw = {"x_affine": c["x_affine"].cuda(), "x_relu": True}
        with _Launches(X.WGRAD_KERNELS, {r.kernel: 1}, tag):
            dW = K.conv2d_wgrad(G, Xt, r.Cout, r.Cin, r.k, r.k, r.stride, r.pad, **kw)
        assert dW.dtype == torch.float32
        X.assert_exact(dW, c["want"], tag, axes=X.WGRAD_AXES, hists=X.WGRAD_HISTS)
        if form == "slices":      # the same slices through the C ABI's own g_coff / x_coff (above: folded into the pointers, as the model does)
            with _Launches(X.WGRAD_KERNELS, {r.kernel: 1}, tag + "/coff"):
                dW = K.conv2d_wgrad(Gw, Xw, r.Cout, r.Cin, r.k, r.k, r.stride, r.pad, g_coff=c["g_coff"], cg=c["cg"],
                                    x_coff=c["x_coff"], cx=r.Cin)
            X.assert_exact(dW, c["want"], tag + "/coff", axes=X.WGRAD_AXES, hists=X.WGRAD_HISTS)


def _ids(pairs):
    return [f"{r.name}-{dt}" for r, dt in pairs]


_FWD = [(r, dt) for r in X.ROWS for dt in r.dtypes]
_TCONV = [(r, dt) for r in X.TCONV_ROWS for dt in r.dtypes]
_AFFINE = [(r, dt) for r in X.AFFINE_ROWS for dt in r.dtypes]
_WGRAD = [(r, dt) for r in X.WROWS for dt in r.dtypes]


@pytest.mark.parametrize("r,dt", _FWD, ids=_ids(_FWD))
def test_forward_exact(r, dt):
    """Plain, statistics rows per 8x16 tile, bias + ReLU, scale + bias + addend + ReLU, channel slices on both sides."""
    run_forward(r, dt, X.FWD_FORMS)


@pytest.mark.parametrize("r,dt", _AFFINE, ids=_ids(_AFFINE))
def test_forward_input_affine_exact(r, dt):
    """The patch kernel reading relu(x * scale + shift): power-of-two scales and integer shifts keep the staged input exact."""
    assert _k().fused_input_ok(TORCH_DT[dt], r.B, r.H, r.W, r.Cin, r.Cout, 3, 3, 1, 1)
    run_forward(r, dt, ("in_affine_relu",))


@pytest.mark.parametrize("r,dt", _FWD, ids=_ids(_FWD))
def test_dgrad_exact(r, dt):
    """Plain, addend, addend + ReLU; the result buffer is pre-filled, so every pixel must be written."""
    run_dgrad(r, dt, X.DGRAD_FORMS)


@pytest.mark.parametrize("r,dt", _TCONV, ids=_ids(_TCONV))
def test_transposed_conv_forward_exact(r, dt):
    """ConvTranspose2d k3 s2 p1 op1 through the data-gradient launch: four stride phases, three on the patch kernel."""
    run_dgrad(r, dt, ("plain",))


@pytest.mark.parametrize("r,dt", _WGRAD, ids=_ids(_WGRAD))
def test_wgrad_exact(r, dt):
    """fp32 result, exact below 2^24: the generic kernel, the nine-tap kernel (plain, channel slices on both operands,
    accumulate onto an integer-valued dW, x_affine + ReLU) and the ConvTranspose2d weight layout."""
    run_wgrad(r, dt)


@pytest.mark.parametrize("shape,mode,c_pad", [((24, 16, 3, 3), 0, 16), ((24, 16, 3, 3), 1, 24), ((9, 40, 1, 1), 0, 40),
                                              ((9, 40, 1, 1), 1, 16), ((32, 3, 5, 5), 0, 8), ((25, 128, 1, 1), 1, 32),
                                              ((200, 8, 3, 3), 1, 200), ((64, 64, 3, 3), 0, 64)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pack_weight_exact(shape, mode, c_pad, dt):
    """Mode 0 and mode 1 with channel padding: the padding is zeros, every weight is where the kernels look for it."""
    w = X.int_tensor(torch.Generator().manual_seed(sum(shape) + mode), shape, 3, 0.9)
    _packed(w, mode, c_pad, dt, f"pack{shape}")


def run_table(name):
    """Child-process entry: every row of CHILD_TABLES[name], forward and data gradient, all forms."""
    _, rows = X.CHILD_TABLES[name]
    n = 0
    for r in rows:
        for dt in r.dtypes:
            run_forward(r, dt, X.FWD_FORMS)
            run_dgrad(r, dt, X.DGRAD_FORMS)
            n += 1
    torch.cuda.synchronize()
    print(f"exact ok: {name}, {n} cases")


@pytest.mark.parametrize("name", sorted(X.CHILD_TABLES))
def test_switched_kernels_exact_in_a_child_process(name):
    """The library reads its switches once per process: K2r and K2q at tiny rasters (their MIN switches at 1: less than one
    tile, one tile, ragged, a workgroup's run crossing images) and the 8-wave 256 x 128 tile (JSPSR_CONV_TALL=2) run in a
    child that imports this module; the census there proves conv64_resident / conv128_resident / conv_patch_16x16x128."""
    env, rows = X.CHILD_TABLES[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"from tests.test_conv_exact_gpu import run_table; run_table({name!r})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=root)
    n = sum(len(row.dtypes) for row in rows)
    assert r.returncode == 0 and f"exact ok: {name}, {n} cases" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
