"""The bit-exact convolution tests, the part that needs no GPU: every case of tests/test_conv_exact_gpu.py satisfies the
conditions under which its comparison is exact and sees (nearly) every element, the fp32 CPU reference agrees with fp64
wherever fp64 is affordable, and the gap the exact tests close -- localised errors that the relative-Frobenius criterion of
the norm tests accepts -- stated as a test."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_exact_ref as X

_FWD = [(r, X.FWD_FORMS) for r in X.ROWS + X.K2R_TINY_ROWS + X.K2Q_TINY_ROWS + X.TALL2_ROWS] + \
       [(r, ("in_affine_relu",)) for r in X.AFFINE_ROWS]
_DGRAD = [(r, X.DGRAD_FORMS) for r in X.ROWS + X.K2R_TINY_ROWS + X.K2Q_TINY_ROWS + X.TALL2_ROWS] + \
         [(r, ("plain",)) for r in X.TCONV_ROWS]


def test_every_row_has_a_unique_name_and_states_its_kernels():
    rows = X.ROWS + X.TCONV_ROWS + X.AFFINE_ROWS + X.K2R_TINY_ROWS + X.K2Q_TINY_ROWS + X.TALL2_ROWS
    assert len({r.name for r in rows}) == len(rows)
    for r in rows:
        for census in (r.fwd, r.dgrad):
            assert census is None or (census and set(census) <= set(X.CONV_KERNELS)), r.name
        assert r.fwd or r.dgrad, r.name
        assert all(r.Cin % X.epc(d) == 0 for d in r.dtypes), r.name
    assert len({r.name for r in X.WROWS}) == len(X.WROWS)
    assert all(r.kernel in X.WGRAD_KERNELS for r in X.WROWS)
    # every launch name of the census is the stated kernel of some case
    stated = set()
    for r in rows:
        stated |= set(r.fwd or ()) | set(r.dgrad or ())
    assert stated == set(X.CONV_KERNELS) and {r.kernel for r in X.WROWS} == set(X.WGRAD_KERNELS)


@pytest.mark.parametrize("r,forms", _FWD, ids=[r.name for r, _ in _FWD])
def test_forward_cases_meet_the_preconditions(r, forms):
    for form in forms:
        c = X.forward_case(r, form)
        for dt in r.dtypes:
            X.preconditions(c, dt)
        oh, ow = X.out_hw(r)
        assert c["want"].shape == (r.B, oh, ow, r.Cout)
        if form == "stats":
            assert c["stats"].shape == (r.B * ((oh + 7) // 8) * ((ow + 15) // 16), 2, r.Cout)
            assert c["stats_pairs"] == (r.name.startswith("patch_16x16"))
            # the paired numbering and the plain one fold to the same, independently summed, 16x16 tiles
            for st in (c["stats"], X.tile_rows(c["conv"])):
                assert torch.equal(X.fold_rows16(st, r.B, oh, ow), c["stats16"])


@pytest.mark.parametrize("r,forms", _DGRAD, ids=[r.name for r, _ in _DGRAD])
def test_dgrad_cases_meet_the_preconditions(r, forms):
    for form in forms:
        c = X.dgrad_case(r, form)
        for dt in r.dtypes:
            X.preconditions(c, dt)
        assert c["want"].shape == (r.B, r.H, r.W, r.Cout)
        assert (c["conv"][:, ~c["reach"]] == 0).all()


@pytest.mark.parametrize("r", X.WROWS, ids=[r.name for r in X.WROWS])
def test_wgrad_cases_meet_the_preconditions(r):
    for form in r.forms:
        for dt in r.dtypes:
            c = X.wgrad_case(r, form, dt)
            X.preconditions(c, dt)
            assert c["want"].shape == (r.Cout, r.Cin, r.k, r.k) and c["cg"] % X.epc(dt) == 0


def test_fp64_is_taken_wherever_it_is_affordable():
    """_both_precisions asserts fp32 == fp64 bit for bit inside every builder; this pins which rows it covers: all but the
    250 x 255 rasters of the 16x16-tile rows (7 to 14 G multiply-adds) and K2q's 2048 tiles (39 G)."""
    no64 = {r.name for r in X.ROWS + X.TALL2_ROWS if not X.has_fp64(r)}
    assert no64 == {"patch_16x16_f32", "patch_16x16_bf16", "patch_16x16_wide", "patch_16x16x128", "k2q_2048_tiles"}
    assert all(X.has_fp64(r) for r in X.TCONV_ROWS + X.AFFINE_ROWS + X.K2R_TINY_ROWS + X.K2Q_TINY_ROWS)
    # and a reference that is NOT exact is noticed: one non-integer operand of full fp32 precision
    x = torch.full((1, 64, 8, 8), 1.0 / 3.0)
    w = torch.full((8, 64, 3, 3), 1.0 / 7.0)
    with pytest.raises(AssertionError, match="not exact"):
        X._both_precisions(lambda a, b: F.conv2d(a, b, None, 1, 1), 1e6, x, w)


def test_int_tensor():
    g = torch.Generator().manual_seed(1)
    t = X.int_tensor(g, (64, 64, 16), 2, 0.25)
    assert t.dtype == torch.float32 and torch.equal(t, t.round()) and t.abs().max() == 2
    assert 0.17 < (t != 0).float().mean() < 0.23           # 0.25 * 4/5
    assert torch.equal(t.bfloat16().float(), t)
    assert torch.equal(t, X.int_tensor(torch.Generator().manual_seed(1), (64, 64, 16), 2, 0.25))


def test_a_broken_case_fails_its_preconditions():
    r = X.ROWS[0]
    c = dict(X.forward_case(r, "plain"))
    c["stored"] = [c["want"] * 8]
    with pytest.raises(AssertionError, match="stored"):
        X.preconditions(c, "bf16")
    c = dict(X.forward_case(r, "plain"))
    c["pre_relu"] = c["want"] * (torch.rand(c["want"].shape) < 0.5)
    with pytest.raises(AssertionError, match="non-zero share"):
        X.preconditions(c, "f32")
    c = dict(X.forward_case(r, "bias_relu"))
    c["pre_relu"] = c["pre_relu"].abs() + 1
    with pytest.raises(AssertionError, match="clipped"):
        X.preconditions(c, "f32")


def test_assert_exact_names_the_coordinates_of_a_single_wrong_element():
    want = X.forward_case(X.ROWS[2], "plain")["want"]          # (2, 17, 35, 40)
    got = want.clone()
    got[1, 16, 34, 39] += 1
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got.bfloat16(), want, "planted")
    msg = str(e.value)
    v = want[1, 16, 34, 39].item()
    assert "planted: 1 of" in msg and f"(1, 16, 34, 39, {v + 1:g}, {v:g})" in msg
    assert "by y % 16: {0: 1}" in msg and "by x % 16: {2: 1}" in msg and "by c % 64: {39: 1}" in msg
    assert "by b: {1: 1}" in msg and "edge of the y-x raster: 1, interior: 0" in msg
    X.assert_exact(want.bfloat16(), want, "clean")
    with pytest.raises(AssertionError, match="1 of"):                                      # NaN never compares equal
        X.assert_exact(torch.where(got != want, torch.full_like(got, float("nan")), got), want, "nan")


def test_assert_exact_labels_other_tensors_by_their_own_axes():
    want = torch.zeros(6, 5, 2, 8)
    got = want.clone()
    got[4, 3, 1, 7] = 1
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got, want, "rows", axes=X.STATS_AXES, hists=X.STATS_HISTS)
    msg = str(e.value)
    assert "by tile column: {3: 1}" in msg and "by sum|sumsq: {1: 1}" in msg and "edge" not in msg and "% 16" not in msg
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got, want, "dW", axes=X.WGRAD_AXES, hists=X.WGRAD_HISTS)
    assert "by r % 64: {4: 1}" in str(e.value) and "by kx: {7: 1}" in str(e.value) and "edge" not in str(e.value)


def test_localised_errors_pass_the_norm_criterion_and_fail_the_exact_one():
    """The gap.  On the 2 x 256 x 256 x 64 result of the K2r row, three localised corruptions each stay below the 6e-3
    relative Frobenius error that tests/test_conv_gpu.py allows a bf16 result -- so a kernel producing them would pass --
    and each fails assert_exact, whose message points at the corrupted place:
      (a) one 16-pixel row of one tile, all 64 channels, loses one tap (ky = 0, kx = 0);
      (b) the four corner pixels of image 0 come back as zeros in all channels;
      (c) the last column of the last image (256 pixels x 64 channels) loses one 8-channel chunk of the tap (ky = 2, kx = 0).
    How much the norm criterion hides is a matter of energy, 6e-3^2 of the tensor's: about 300 elements wrong by the
    tensor's rms.  Measured on this tensor: zeroing the 1024 elements of (a) gives 1.1e-2 and dropping the whole tap in (c)
    1.5e-2 -- those the old criterion would see -- which is why (a) and (c) drop a tap and a chunk of a tap."""
    r = next(r for r in X.ROWS if r.name == "k2r_512_tiles")
    c = X.forward_case(r, "plain")
    want = c["want"]
    x, w = c["x"], c["w"]                                     # (B,H,W,C), (O,I,3,3)
    B, H, W, C = want.shape

    def tap(ky, kx, b, ys, xs, ci=slice(None)):
        """The contribution of tap (ky, kx), input channels ci, to the output pixels (b, ys, xs): (len(ys), len(xs), 64)."""
        xp = F.pad(x[b], (0, 0, 1, 1, 1, 1))                  # (H+2, W+2, C): padded row iy + 1 holds input row iy
        patch = xp[ys.start + ky:ys.stop + ky, xs.start + kx:xs.stop + kx, ci]
        return patch @ w[:, ci, ky, kx].t()

    corrupt = {}
    a = want.clone()
    ys, xs = slice(8 * 13 + 5, 8 * 13 + 6), slice(16 * 7, 16 * 8)
    a[1, ys, xs] -= tap(0, 0, 1, ys, xs)
    corrupt["a"] = (a, 1024, "by y % 16: {13: ", "by b: {1: ")
    b_ = want.clone()
    for yy in (0, H - 1):
        for xx in (0, W - 1):
            b_[0, yy, xx] = 0
    corrupt["b"] = (b_, 256, "interior: 0", "by b: {0: ")
    c_ = want.clone()
    c_[B - 1, :, W - 1:] -= tap(2, 0, B - 1, slice(0, H), slice(W - 1, W), slice(0, 8))
    corrupt["c"] = (c_, 256 * 64, "by x % 16: {15: ", f"by b: {{{B - 1}: ")
    for key, (t, most, *marks) in corrupt.items():
        n = int((t != want).sum())
        assert most // 4 <= n <= most, (key, n)          # (the operands are sparse: a dropped tap is zero at some pixels)
        rel = X.rel_fro(t.bfloat16().float(), want)
        print(f"corruption ({key}): {n} elements, relative Frobenius error {rel:.2e}")
        assert 0 < rel < 6e-3, (key, rel)                       # the old criterion accepts it
        with pytest.raises(AssertionError) as e:
            X.assert_exact(t.bfloat16(), want, key)
        for m in marks:
            assert m in str(e.value), (key, m, str(e.value))
    # the figures of the docstring: what the old criterion does see
    z = want.clone()
    z[1, ys, xs] = 0
    print(f"zeroing the row of (a): {X.rel_fro(z.bfloat16().float(), want):.2e}")
    assert X.rel_fro(z.bfloat16().float(), want) > 6e-3
    d = want.clone()
    d[B - 1, :, W - 1:] -= tap(2, 0, B - 1, slice(0, H), slice(W - 1, W))
    print(f"dropping the whole tap in (c): {X.rel_fro(d.bfloat16().float(), want):.2e}")
    assert X.rel_fro(d.bfloat16().float(), want) > 6e-3
