"""The exact tests of the per-channel kernels (K4/K5), the part that needs no GPU: every case of
tests/test_perchannel_exact_gpu.py meets the conditions under which its comparison is exact, every exact reference has
the same bits when it is evaluated in float32 with its sums in another order (so a kernel is free to order them), every
mutant of tests/perchannel_exact_ref.py is caught by the new comparison, the gap to the relative-Frobenius criterion of
tests/test_elementwise_gpu.py is recorded, and the workspace every entry point writes fits the bytes promised."""
import pytest
import torch

from tests import perchannel_exact_ref as X

_IDS = [X.geo_id(g) for g in X.GEOS + X.CHILD_GEOS]
_POW2 = lambda g: ((g.B * g.H * g.W) & (g.B * g.H * g.W - 1)) == 0


def test_tables_reach_the_geometries_they_name():
    for dt in ("f32", "bf16"):
        v = X.VEC[dt]
        assert [c // v for c in X.CHANNELS[dt]] == [1, 3, 5, 16 if dt == "f32" else 8, 48 if dt == "f32" else 24, 64, 65,
                                                   384 if dt == "f32" else 192]
        assert X.make_red(64, 1, X.CHANNELS[dt][6], v)["gy"] == 2          # 65 groups: one lane in the second blockIdx.y
        for C in X.CHANNELS[dt]:
            rs = X.rasters(dt, C)
            npix = [b * h * w for b, h, w in rs]
            chunks = [X.make_red(n, 1, C, v)["chunks"] for n in npix]
            assert len(rs) >= 3 and any(n & (n - 1) for n in npix) and any(n & (n - 1) == 0 for n in npix) and max(chunks) > 1
            assert any(ch > 1 and X.make_red(n, 1, C, v)["chunk_pix"] * ch != n for n, ch in zip(npix, chunks)), "no ragged last chunk"
            assert ((1, 64, 64) in rs) == (C <= 256)
        # up to 8 groups under the default block target: the tail loop only (a chunk has at most 64 pixels below 4096, a
        # trip of the main loop needs 3 * 4 * pl + 1); the child table runs the main loop at 64 pixels side by side
        for C in [c for c in X.NARROW[dt] if c // v <= 8]:
            assert not any(X.main_loop_runs(b * h * w, 1, C, v) for b, h, w in X.rasters(dt, C) if b * h * w < 4096)
        assert X.make_red(2500, 1, X.NARROW[dt][0], v)["pl"] == 64
    for g in X.CHILD_GEOS:
        r = X.make_red(2500, 1, g.C, X.VEC[g.dt], 2)
        assert r["chunks"] == 2 and r["chunk_pix"] == 1250 and X.main_loop_runs(2500, 1, g.C, X.VEC[g.dt], 2)
    assert max(g.B * g.H * g.W * g.C for g in X.GEOS) == 4096 * 256
    for dt, ws in X.SLICE_WIDTHS.items():
        assert len(ws) >= 2 and set(ws) <= set(X.CHANNELS[dt])


@pytest.mark.parametrize("geo", X.GEOS + X.CHILD_GEOS, ids=_IDS)
def test_batchnorm_and_relu_cases_meet_the_preconditions(geo):
    for variant in X.BN_VARIANTS:
        X.preconditions(X.bn_eval_case(geo, variant), geo.dt)
        X.preconditions(X.bn_train_case(geo, variant), geo.dt)
    for mode in X.BWD_MODES:
        for training in (False, True):
            c = X.bn_bwd_case(geo, mode, training)
            assert c["exact"] == (not training or _POW2(geo))
            X.preconditions(c, geo.dt)
    for relu in (False, True):
        X.preconditions(X.act_case(geo, relu), geo.dt)


@pytest.mark.parametrize("geo", X.GEOS + X.CHILD_GEOS, ids=_IDS)
def test_gate_cases_meet_the_preconditions(geo):
    for form in X.GATE_FORMS:
        if form == "ties" and geo.H * geo.W < 4:
            continue
        X.preconditions(X.gate_case(geo, form), geo.dt)
    if (geo.H, geo.W) == (5, 7):
        X.preconditions(X.gate_case(geo, "ties", 3), geo.dt)


@pytest.mark.parametrize("shape", X.MLP_SHAPES, ids=str)
def test_gate_mlp_cases_meet_the_preconditions(shape):
    X.preconditions(X.mlp_case(*shape), "f32")


@pytest.mark.parametrize("geo", X.GEOS + X.CHILD_GEOS, ids=_IDS)
def test_exact_references_do_not_depend_on_the_summation_order(geo):
    """The BatchNorm backward (the one operator here whose result is not a sum of integers) evaluated in float32 with its two
    sums taken over the pixels in two shuffled orders: the same bits as the fp64 reference.  With the preconditions (every
    intermediate is a float32 number) this is why a zero tolerance is fair to a kernel that sums in its own order."""
    n = geo.B * geo.H * geo.W
    gen = torch.Generator().manual_seed(n + geo.C)
    for mode in X.BWD_MODES:
        for training in (False, True):
            c = X.bn_bwd_case(geo, mode, training)
            if not c["exact"]:
                continue
            for _ in range(2):
                f = X.bn_bwd_case(geo, mode, training, dtype=torch.float32, perm=torch.randperm(n, generator=gen))
                for k in ("dx", "dgamma", "dbeta", "dz"):
                    assert f[k].dtype == torch.float32 and torch.equal(f[k].double(), c[k]), (mode, training, k)
    # the eval-mode forward, float32, with and without the shift folded first, and the residual joined in either order
    for variant in X.BN_VARIANTS:
        c = X.bn_eval_case(geo, variant)
        x, sc, sh, mu = c["x"].float(), c["scale"].float(), c["shift"].float(), c["mean"].float()
        bn_a, bn_b = x * sc + sh, (x - mu) * sc + c["beta"].float()
        assert torch.equal(bn_a, bn_b)
        if c["with_res"]:
            r = c["res"].float() * c["raff"][0].float() + c["raff"][1].float() if c["with_raff"] else c["res"].float()
            bn_a = bn_a * c["res_scale"] + r
        assert torch.equal(X.store((torch.relu(bn_a) if c["relu"] else bn_a).double(), geo.dt), c["y"]), variant
    # the gate's backward apply, float32, in both association orders
    c = X.gate_case(geo, "random")
    r = X.gate_apply_ref(c, geo.dt)
    if r["exact"]:
        dy, s, dm = c["dy"].float(), c["s"].float().unsqueeze(1), (c["hit"] * c["dmax"].unsqueeze(1)).float()
        da = (c["davg"].float() * (1.0 / torch.tensor(float(c["npix"])))).unsqueeze(1)
        assert torch.equal(((dy * s + da) + dm).double(), r["dx"]) and torch.equal((dy * s + (da + dm)).double(), r["dx"])


def _caught(fn):
    with pytest.raises(AssertionError):
        fn()


def test_every_mutant_is_caught_by_the_exact_comparison():
    """Each mutant on the reference of a bf16 case: the comparison of the GPU tests (check_exact / the sentinel check) fails."""
    geo = X.Geo("bf16", 24, 2, 9, 11)
    good = X.bn_bwd_case(geo, "1y_dres", False)
    bad = X.MUTANTS["drop_last_pixel_of_chunks"](geo, "1y_dres", False)
    X.check_exact(X.store(good["dgamma"], "f32"), good["dgamma"], "self")
    _caught(lambda: X.check_exact(X.store(bad["dbeta"], "f32"), good["dbeta"], "dbeta"))
    _caught(lambda: X.check_exact(X.store(bad["dgamma"], "f32"), good["dgamma"], "dgamma"))
    geo2 = X.Geo("bf16", 24, 1, 16, 16)      # training mode, power of two: the sums reach dx too
    good2, bad2 = X.bn_bwd_case(geo2, "1y_dres", True), X.MUTANTS["drop_last_pixel_of_chunks"](geo2, "1y_dres", True)
    _caught(lambda: X.check_exact(X.store(bad2["dx"], "bf16"), good2["dx"], "dx", "bf16"))
    dx = X.store(good2["dx"], "bf16")
    for name in ("swap_channels_in_group", "shift_lane_group"):
        _caught(lambda: X.check_exact(X.MUTANTS[name](dx, "bf16"), good2["dx"], name, "bf16"))
    y = X.bn_eval_case(geo, "res_relu_mask")["y"]
    for name in ("swap_channels_in_group", "shift_lane_group"):
        _caught(lambda: X.check_exact(X.MUTANTS[name](y, "bf16"), y, name, "bf16"))
    c = X.gate_case(geo, "ties")
    _caught(lambda: X.check_exact(X.MUTANTS["last_argmax"](c), c["amax"], "amax"))
    t = X.bn_train_case(geo, "plain")
    rows = X.partial_rows(t, 300)
    m_bad = (X.MUTANTS["fold_drops_final_row"](rows)[0] / t["npix"]).float()
    _caught(lambda: X.check_exact(m_bad, t["save_mean"], "save_mean"))
    buf = torch.full((2, 9, 11, 24 + X.SLICE_PAD), 7.0)
    rest = lambda b: torch.cat((b[..., :X.SLICE_OFF], b[..., X.SLICE_OFF + 24:]), 3)
    assert (rest(buf) == 7.0).all() and not (rest(X.MUTANTS["write_outside_slice"](buf, X.SLICE_OFF, 24)) == 7.0).all()


def test_the_norm_criterion_accepts_what_the_exact_one_rejects(capsys):
    """The gap being closed, on the largest shape of tests/test_elementwise_gpu.py (8 x 128 x 128 x 64, bf16; the gate's
    8 x 64 x 64 x 256), under that file's own tolerances (dx / dgamma / dbeta 1.5e-2, the gate's dx 1e-2, statistics 1e-5).
    Accepted by the old criterion, rejected by the exact one: a dx with one wrong element (1.7e-4); a reduce pass that drops
    the last pixel of ONE chunk, on every output (dx 2.4e-4, dbeta 2.6e-3, dgamma 1.8e-3); a reduce pass that drops the last
    pixel of EVERY chunk (1 pixel in 128), on dx (6.7e-3).  Visible to the old criterion too, and said here rather than
    bent: dropping a pixel of every chunk moves dbeta / dgamma (sums with random signs) by 9 % of their norm; two swapped
    channels or a shifted lane group over the WHOLE tensor are 2 and 8 channels of 64 (0.16, 0.59); the last argmax moves
    a dmax of 1-3 beside gradients of the same size (5e-2); a fold without its final row is plain wrong.  Those four were
    invisible only because no test compared the tensor in question (amax, partial=, ext_partial=) or ran the path at
    all."""
    geo = X.Geo("bf16", 64, 8, 128, 128)
    n = geo.B * geo.H * geo.W
    good = X.bn_bwd_case(geo, "1y_dres", True)
    dx = X.store(good["dx"], "bf16")
    report = {}
    one = dx.clone()
    one[3, 77, 5, 9] += 1.0
    report["one_element/dx"] = X.old_criterion(one, dx, 1.5e-2)
    for name in ("swap_channels_in_group", "shift_lane_group"):
        report[name + "/dx"] = X.old_criterion(X.MUTANTS[name](dx, "bf16"), dx, 1.5e-2)
    every = X.MUTANTS["drop_last_pixel_of_chunks"](geo, "1y_dres", True)
    keep = torch.ones(n)
    keep[X.make_red(n, 1, 64, 8)["chunk_pix"] - 1] = 0
    single = X.bn_bwd_case(geo, "1y_dres", True, keep=keep)
    for tag, m in (("every_chunk", every), ("one_chunk", single)):
        report[f"drop_last_pixel/{tag}/dx"] = X.old_criterion(X.store(m["dx"], "bf16") if X.is_f32(m["dx"]) else m["dx"].float().bfloat16().float(), dx, 1.5e-2)
        report[f"drop_last_pixel/{tag}/dbeta"] = X.old_criterion(m["dbeta"], good["dbeta"], 1.5e-2)
        report[f"drop_last_pixel/{tag}/dgamma"] = X.old_criterion(m["dgamma"], good["dgamma"], 1.5e-2)
    g8 = X.gate_case(X.Geo("bf16", 256, 8, 64, 64), "random")
    r = X.gate_apply_ref(g8, "bf16")
    hit_bad = torch.zeros_like(g8["hit"])
    hit_bad.scatter_(1, X.MUTANTS["last_argmax"](g8).long().unsqueeze(1), 1.0)
    dx_bad = r["dx"] + (hit_bad - g8["hit"]) * g8["dmax"].unsqueeze(1)
    report["last_argmax/gate dx"] = X.old_criterion(dx_bad, r["dx"], 1e-2)
    t = X.bn_train_case(geo, "plain")
    rows = X.partial_rows(t, 300)
    report["fold_drops_final_row/mean"] = X.old_criterion(X.MUTANTS["fold_drops_final_row"](rows)[0] / n, t["save_mean"], 1e-5)
    wide = torch.full((8, 128, 128, 64 + X.SLICE_PAD), 7.0)
    report["write_outside_slice/whole buffer"] = X.old_criterion(X.MUTANTS["write_outside_slice"](wide, X.SLICE_OFF, 64), wide, 5e-3)
    with capsys.disabled():
        for k, (v, ok) in report.items():
            print(f"\n  old criterion, {k}: rel_fro {v:.3e} -> {'passes' if ok else 'fails'}", end="")
        print()
    # the exact comparison rejects each of them
    _caught(lambda: X.check_exact(one, good["dx"], "one element", "bf16"))
    _caught(lambda: X.check_exact(single["dbeta"].float(), good["dbeta"], "dbeta"))
    # ... and the old one accepts these
    for k in ("one_element/dx", "write_outside_slice/whole buffer", "drop_last_pixel/every_chunk/dx", "drop_last_pixel/one_chunk/dx", "drop_last_pixel/one_chunk/dbeta", "drop_last_pixel/one_chunk/dgamma"):
        assert report[k][1], (k, report[k])


def test_workspace_every_entry_point_fits_the_bytes_promised():
    """include/jspsr_hip.h's table against jspsr_reduce_workspace_bytes, for every width of the tables plus 1792 and 2048
    (fp32) and 3584 (bf16), under the default block target and small ones: what an entry point may write is at most what
    the query promises.  (Before the forward's 256 external rows were counted the query returned (3 rows + 4) C floats
    and this failed from 7 channel blocks on: fp32 C = 1792 promised 442 C floats where bn_forward(partial=) of 256 or
    more rows writes 514 C.)"""
    from jspsr_amd import _lib
    lib = _lib.load()
    for dt, code in (("f32", 0), ("bf16", 1)):
        for C in X.CHANNELS[dt] + X.WORKSPACE_EXTRA[dt]:
            for nseg in (1, 3, 8):
                promised = lib.jspsr_reduce_workspace_bytes(code, C, nseg)
                assert promised == X.promised_floats(dt, C, nseg) * 4 + 64, (dt, C, nseg)      # the mirror is the library's formula
                for target in (1024, 64, 2, 1):
                    p = X.promised_floats(dt, C, nseg, target)
                    for npix in (1, 35, 64, 198, 4096, 2500, 1 << 20, 1 << 31):
                        writes = [X.written_floats(e, dt, C, nseg, npix, target) for e in ("act_backward", "gate_pool", "gate_backward_reduce")]
                        if nseg == 1:
                            writes += [X.written_floats("bn_forward", dt, C, 1, npix, target, r) for r in (0,) + X.PARTIAL_ROWS]
                            writes += [X.written_floats("bn_backward", dt, C, 1, npix, target, r) for r in (0,) + X.EXT_ROWS]
                        assert max(writes) <= p, (dt, C, nseg, target, npix, max(writes), p)
    # the case of the issue, and that the old formula is what fell short
    assert X.written_floats("bn_forward", "f32", 1792, 1, 16, ext_rows=300) == 514 * 1792
    assert X.promised_floats("f32", 1792, 1, parent=True) == 442 * 1792 < 514 * 1792 <= X.promised_floats("f32", 1792, 1)
    assert X.promised_floats("f32", 1536, 1, parent=True) == 514 * 1536
