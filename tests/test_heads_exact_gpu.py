"""GPU: the two output heads -- K1c (csrc/head.hip: jspsr_head_forward / jspsr_head_backward) and K1p (csrc/head1.hip:
jspsr_conv_head1_*) -- on integer operands, compared element by element with plain torch on the CPU at zero tolerance
(tests/heads_exact_ref.py has the operands, the references and the reasons the arithmetic is exact).  Every case goes
through the C ABI, pre-fills its results with 7, checks the bytes beside every slice, gives the backward a workspace of
exactly the promised bytes followed by a canary page, and proves its launches with the census before and after.  What
this pins is indexing: planes, pixels, channel halves, the grid-stride loop's later trips, tiles, bands, halos, idle lanes."""
import os
import subprocess
import sys

import pytest
import torch

from tests import heads_exact_ref as H
from tests.test_conv_exact_gpu import _Launches

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ES = {"f32": 4, "bf16": 2}
CANARY, PATTERN = 4096, 0xA5


def _L():
    from jspsr_amd import _lib
    return _lib


def _dt(dt):
    from jspsr_amd import kernels as K
    return K.F32 if dt == "f32" else K.BF16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _per_cu():
    return int(os.environ.get("JSPSR_HEAD_WGS", "4"))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _filled(shape, dtype=torch.float32):
    return torch.full(tuple(shape), H.FILL, dtype=dtype, device="cuda")


def _workspace(nbytes):
    """Exactly the promised bytes, then a canary page; all of it a byte pattern no integer sum has."""
    ws = torch.empty(nbytes + CANARY, dtype=torch.uint8, device="cuda")
    ws.fill_(PATTERN)
    return ws


def _beside(t, coff, C, tag):
    rest = torch.cat((t[..., :coff], t[..., coff + C:]), 3)
    assert (rest == H.FILL).all(), f"{tag}: wrote outside the channel slice"


# ---- K1c ------------------------------------------------------------------------------------------------------------------
def k1c_forward(x_ptr, cs, coff, c, dt, tag):
    """jspsr_head_forward on the case's weights -> planes, launched once."""
    L = _L()
    lib = L.load()
    B, Hh, W = c["shape"]
    w, b = c["w"].cuda(), c["b"].cuda()
    planes = _filled((B, H.NP, Hh, W))
    assert lib.jspsr_head_ok(_dt(dt), B, Hh, W, c["cin"]) == 1, tag       # the accepting side of head_ok's agreement with the entry
    with _Launches(H.LAUNCH_NAMES, {"head_forward": 1}, tag):
        L.check(lib.jspsr_head_forward(_dt(dt), x_ptr, cs, coff, c["cin"], w.data_ptr(), b.data_ptr(), planes.data_ptr(),
                                       B, Hh, W, _stream()), tag)
    torch.cuda.synchronize()
    return planes


def k1c_backward(c, dt, want_dx, tag):
    """jspsr_head_backward: dx into channels [16, 16 + Cin) of a wider buffer (or none), gn, db; the workspace is exactly
    the promised bytes, and the rows written are the grid the rule gives -> (dx_wide | None, gn, db)."""
    L = _L()
    lib = L.load()
    B, Hh, W = c["shape"]
    cin, tdt = c["cin"], TORCH_DT[dt]
    w, g = c["w"].cuda(), c["g"].cuda()
    dxw = _filled((B, Hh, W, cin + H.DX_EXTRA), tdt) if want_dx else None
    gn, db = _filled((B, Hh, W, 32), tdt), _filled((H.NP,))
    nbytes = lib.jspsr_head_backward_workspace_bytes(B, Hh, W)
    ws = _workspace(nbytes)
    groups = B * Hh * W // 32
    rows = H.head_grid_rows(groups, _cus(), _per_cu())
    assert rows * 32 * 4 <= nbytes, f"{tag}: {rows} partial rows do not fit the workspace: not launched"
    with _Launches(H.LAUNCH_NAMES, {"head_backward": 1, "head_dbias_fold": 1}, tag):
        L.check(lib.jspsr_head_backward(_dt(dt), g.data_ptr(), w.data_ptr(), cin, dxw.data_ptr() if want_dx else None,
                                        cin + H.DX_EXTRA if want_dx else 0, H.DX_COFF if want_dx else 0, gn.data_ptr(),
                                        db.data_ptr(), ws.data_ptr(), B, Hh, W, _stream()), tag)
    torch.cuda.synchronize()
    assert (ws[nbytes:] == PATTERN).all(), f"{tag}: wrote past the bytes jspsr_head_backward_workspace_bytes promises"
    written = (ws[:nbytes].view(-1, 128) != PATTERN).any(1).nonzero().flatten().tolist()
    assert written == list(range(rows)), f"{tag}: partial rows written {written[:8]}.. ({len(written)}), the grid rule gives {rows}"
    return dxw, gn, db


def run_k1c(shape, cin, dt, forms=H.K1C_FORMS, routes=True):
    tdt = TORCH_DT[dt]
    for form in forms:
        c = H.head_case(shape, cin, form)
        H.preconditions(c, dt)
        tag = f"k1c{shape}/{cin}/{dt}/{form}"
        x = c["x"].cuda().to(tdt)
        planes = k1c_forward(x.data_ptr(), cin, 0, c, dt, tag + "/fwd dense")
        H.check(planes, c["planes"], tag + "/fwd dense", H.planes_view)
        if routes:
            xw = H.wide(c["x"], H.X_COFF, H.X_EXTRA, 1).cuda().to(tdt)
            cs = cin + H.X_EXTRA
            planes = k1c_forward(xw.data_ptr() + H.X_COFF * ES[dt], cs, 0, c, dt, tag + "/fwd slice by pointer")
            H.check(planes, c["planes"], tag + "/fwd slice by pointer", H.planes_view)
            planes = k1c_forward(xw.data_ptr(), cs, H.X_COFF, c, dt, tag + "/fwd slice by x_coff")
            H.check(planes, c["planes"], tag + "/fwd slice by x_coff", H.planes_view)
        dxw, gn, db = k1c_backward(c, dt, True, tag + "/bwd dx")
        H.check(dxw[..., H.DX_COFF:H.DX_COFF + cin], c["dx"], tag + "/bwd dx: dx", H.pix_view)
        _beside(dxw, H.DX_COFF, cin, tag + "/bwd dx")
        H.check(gn, c["gn"], tag + "/bwd dx: gn (all 32 channels)", H.pix_view)
        H.check(db, c["db"], tag + "/bwd dx: db", H.row_view)
        _, gn0, db0 = k1c_backward(c, dt, False, tag + "/bwd no dx")
        H.check(gn0, c["gn"], tag + "/bwd no dx: gn (all 32 channels)", H.pix_view)
        H.check(db0, c["db"], tag + "/bwd no dx: db", H.row_view)
        assert torch.equal(gn0, gn) and torch.equal(db0, db), f"{tag}: grad_x = NULL changes gn / db"
        if routes:
            k1c_through_ops(c, x, tag + "/ops")


def k1c_through_ops(c, x, tag):
    """ops.head_planes and its backward: the weight gradient through the 1x1 route of the weight-gradient kernel with
    Cg = 32 (the NHWC copy), beside planes, dx and db once more."""
    from jspsr_amd import ops
    cin = c["cin"]
    xd = x.clone().requires_grad_()
    w4 = c["w"].cuda().reshape(H.NP, cin, 1, 1)
    ps = [w4[:9].clone().requires_grad_(), c["b"][:9].cuda().requires_grad_(), w4[9:].clone().requires_grad_(),
          c["b"][9:].cuda().requires_grad_()]
    with _Launches(H.LAUNCH_NAMES, {"head_forward": 1, "head_backward": 1, "head_dbias_fold": 1}, tag):
        planes = ops.head_planes(xd, *ps)
        planes.backward(c["g"].cuda())
        torch.cuda.synchronize()
    H.check(planes, c["planes"], tag + ": planes", H.planes_view)
    H.check(xd.grad, c["dx"], tag + ": dx", H.pix_view)
    H.check(torch.cat((ps[1].grad, ps[3].grad)), c["db"], tag + ": db", H.row_view)
    dW = torch.cat((ps[0].grad, ps[2].grad)).reshape(H.NP, cin)
    assert dW.dtype == torch.float32
    H.check(dW, c["dW"], tag + ": dW", H.row_view)


_K1C = [(s, cin, dt) for s in H.K1C_SHAPES for cin in H.K1C_CINS for dt in H.DTYPES]


@pytest.mark.parametrize("shape,cin,dt", _K1C, ids=[f"{s[0]}x{s[1]}x{s[2]}-c{c}-{d}" for s, c, d in _K1C])
def test_k1c_exact(shape, cin, dt):
    """Forward dense, as a slice by pointer and by x_coff with a wider pitch; backward into a dx slice (gx_coff, wider
    pitch) and with grad_x = NULL (same gn and db bits); gn compared whole; dW through ops.  random and onehot forms."""
    run_k1c(shape, cin, dt)


@pytest.mark.parametrize("cin,dt", [(128, "bf16"), (32, "f32")])
def test_k1c_second_trip_in_process(cin, dt):
    """Just over one sweep of the default grid, sized from the device's CU count: 64 waves take a second trip."""
    cus = _cus()
    shape = H.two_trip_shape(cus, _per_cu())
    groups = shape[1] * shape[2] // 32
    rows = H.head_grid_rows(groups, cus, _per_cu())
    trips = H.head_trips(groups, rows)
    print(f"{cus} CUs: {H.head_groups_per_sweep(cus, _per_cu())} groups per sweep, case {shape} = {groups} groups on {rows} "
          f"workgroups, trips per wave: {trips.count(2)} x 2, {trips.count(1)} x 1")
    assert max(trips) == 2 and trips.count(2) == 64
    run_k1c(shape, cin, dt, forms=("random",), routes=False)


def run_one_workgroup():
    """Child-process entry (JSPSR_HEAD_WGS=0): every width and dtype, both forms, with and without dx, on one workgroup."""
    assert _per_cu() == 0
    n = 0
    for shape in H.ONE_WG_SHAPES:
        groups = shape[0] * shape[1] * shape[2] // 32
        assert H.head_grid_rows(groups, _cus(), 0) == 1
        print(f"one workgroup, {shape}: trips per wave {H.head_trips(groups, 1)}")
        for cin in H.K1C_CINS:
            for dt in H.DTYPES:
                run_k1c(shape, cin, dt)
                n += 1
    torch.cuda.synchronize()
    print(f"exact ok: one workgroup, {n} cases")


def test_k1c_later_trips_exact_in_a_child_process():
    """The library reads JSPSR_HEAD_WGS once per process, and head_grid clamps 0 to a single workgroup: (2, 8, 36) then gives
    its four waves 5, 5, 4 and 4 trips across an image boundary, (1, 4, 8) gives 1, 0, 0 and 0.  k1c_backward proves the
    single workgroup from the one partial row written."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from tests.test_heads_exact_gpu import run_one_workgroup; run_one_workgroup()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **H.ONE_WG_ENV), capture_output=True, text=True,
                       timeout=300, cwd=root)
    print(r.stdout[-2000:])
    n = len(H.ONE_WG_SHAPES) * len(H.K1C_CINS) * len(H.DTYPES)
    assert r.returncode == 0 and f"exact ok: one workgroup, {n} cases" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    assert "(2, 8, 36): trips per wave [5, 5, 4, 4]" in r.stdout and "(1, 4, 8): trips per wave [1, 0, 0, 0]" in r.stdout


# ---- K1p ------------------------------------------------------------------------------------------------------------------
def k1p_backward(c, dt, xw, want_dx, tag):
    L = _L()
    lib = L.load()
    B, Hh, W = c["shape"]
    C, tdt, cs = c["C"], TORCH_DT[dt], c["C"] + H.K1P_EXTRA
    w, dy = c["w"].cuda(), c["dy"].cuda()
    dxw = _filled((B, Hh, W, cs), tdt) if want_dx else None
    dw, db = _filled((1, C, 3, 3)), _filled((1,))
    nbytes = lib.jspsr_conv_head1_workspace_bytes(B, Hh, W, C)
    assert nbytes == H.k1p_tiles(c["shape"]) * (9 * C + 1) * 4
    ws = _workspace(nbytes)
    with _Launches(H.LAUNCH_NAMES, {"head1_backward": 1, "head1_backward_fold": 1}, tag):
        L.check(lib.jspsr_conv_head1_backward(_dt(dt), dy.data_ptr(), xw.data_ptr(), cs, H.K1P_COFF, C, w.data_ptr(),
                                              dxw.data_ptr() if want_dx else None, cs if want_dx else 0,
                                              H.K1P_COFF if want_dx else 0, dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                              B, Hh, W, _stream()), tag)
    torch.cuda.synchronize()
    assert (ws[nbytes:] == PATTERN).all(), f"{tag}: wrote past the bytes jspsr_conv_head1_workspace_bytes promises"
    assert (ws[:nbytes].view(-1, 4) != PATTERN).any(1).all(), f"{tag}: a promised partial sum was not written"
    return dxw, dw, db


def run_k1p(shape, C, dt, forms=None):
    L = _L()
    lib = L.load()
    tdt = TORCH_DT[dt]
    B, Hh, W = shape
    for form in forms or H.k1p_forms(shape):
        c = H.head1_case(shape, C, form)
        H.preconditions(c, dt)
        tag = f"k1p{shape}/{C}/{dt}/{form}"
        xw = H.wide(c["x"], H.K1P_COFF, H.K1P_EXTRA, 2).cuda().to(tdt)
        w, b = c["w"].cuda(), c["b"].cuda()
        y = _filled((B, 1, Hh, W))
        with _Launches(H.LAUNCH_NAMES, {"head1_forward": 1}, tag + "/fwd"):
            L.check(lib.jspsr_conv_head1_forward(_dt(dt), xw.data_ptr(), C + H.K1P_EXTRA, H.K1P_COFF, C, w.data_ptr(),
                                                 b.data_ptr(), y.data_ptr(), B, Hh, W, _stream()), tag + "/fwd")
        torch.cuda.synchronize()
        H.check(y, c["y"], tag + "/fwd: y", H.y_view)
        dxw, dw, db = k1p_backward(c, dt, xw, True, tag + "/bwd dx")
        H.check(dxw[..., H.K1P_COFF:H.K1P_COFF + C], c["dx"], tag + "/bwd dx: dx", None)
        _beside(dxw, H.K1P_COFF, C, tag + "/bwd dx")
        H.check(dw, c["dW"], tag + "/bwd dx: dW", H.row_view)
        H.check(db, c["db"], tag + "/bwd dx: db", H.row_view)
        _, dw0, db0 = k1p_backward(c, dt, xw, False, tag + "/bwd no dx")
        H.check(dw0, c["dW"], tag + "/bwd no dx: dW", H.row_view)
        H.check(db0, c["db"], tag + "/bwd no dx: db", H.row_view)
        assert torch.equal(dw0, dw) and torch.equal(db0, db), f"{tag}: dx = NULL changes dW / db"
        if form == "random":       # and the same bits from run to run
            dxw2, dw2, db2 = k1p_backward(c, dt, xw, True, tag + "/bwd again")
            assert torch.equal(dxw2, dxw) and torch.equal(dw2, dw) and torch.equal(db2, db), f"{tag}: run-to-run bits"


_K1P = [(C, dt) for C in H.K1P_CS for dt in H.DTYPES]


@pytest.mark.parametrize("C,dt", _K1P, ids=[f"c{c}-{d}" for c, d in _K1P])
def test_k1p_exact(C, dt):
    """Every shape the table gives this channel count, random and delta forms; x and dx are channels [8, 8 + C) of C + 16.
    y, dx, dW, db exact; dW / db of the dx = NULL launch and of a repeated launch have the same bits."""
    for shape in H.k1p_shapes(C):
        run_k1p(shape, C, dt)


@pytest.mark.parametrize("dt", H.DTYPES)
def test_workspace_contracts(dt):
    """Both backward entries with a workspace of exactly *_workspace_bytes and a canary page behind it: K1c at its most
    workgroups among the small shapes, K1p at the largest tile count of its table at C = 256."""
    L = _L()
    lib = L.load()
    assert lib.jspsr_head_backward_workspace_bytes(2, 8, 36) == H.HEAD_MAX_WGS * 32 * 4
    c = H.head_case((2, 8, 36), 128, "random")
    dxw, gn, db = k1c_backward(c, dt, True, f"workspace k1c {dt}")
    H.check(db, c["db"], f"workspace k1c {dt}: db", H.row_view)
    shape = max((s for s, cs in H.K1P_TABLE if 256 in cs), key=H.k1p_tiles)
    assert shape == (1, 33, 65)
    c = H.head1_case(shape, 256, "random")
    xw = H.wide(c["x"], H.K1P_COFF, H.K1P_EXTRA, 2).cuda().to(TORCH_DT[dt])
    _, dw, db = k1p_backward(c, dt, xw, True, f"workspace k1p {dt}")
    H.check(dw, c["dW"], f"workspace k1p {dt}: dW", H.row_view)
    H.check(db, c["db"], f"workspace k1p {dt}: db", H.row_view)
