"""The bit-exact tests of the output heads (K1c, K1p), the part that needs no GPU: every case of
tests/test_heads_exact_gpu.py satisfies the conditions under which its comparison is exact, the fp64, int64 and fp32
references agree bit for bit, assert_exact catches every planted fault (and the table of what the tolerance criteria would
have said about each is printed: profiles/r20_heads_exact_suite.txt), K1c's entry points refuse what they must, and the
grid rule the two-trip cases are sized by."""
import ctypes

import pytest
import torch

from tests import heads_exact_ref as H

_K1C = [(s, cin) for s in H.K1C_SHAPES for cin in H.K1C_CINS]
_K1P = [(s, C) for s, cs in H.K1P_TABLE for C in cs]


@pytest.mark.parametrize("shape,cin", _K1C, ids=[f"{s}-{c}" for s, c in _K1C])
def test_k1c_cases_meet_the_preconditions(shape, cin):
    for form in H.K1C_FORMS:
        c = H.head_case(shape, cin, form)
        for dt in H.DTYPES:
            H.preconditions(c, dt)
        assert H.references_agree(c) == 2
        B, Hh, W = shape
        assert c["planes"].shape == (B, 25, Hh, W) and c["dx"].shape == (B, Hh, W, cin) and c["gn"].shape == (B, Hh, W, 32)
        assert (c["gn"][..., 25:] == 0).all() and torch.equal(c["gn"][..., :25], c["g"].permute(0, 2, 3, 1))
        if form == "onehot":       # what the probe promises: one channel per pixel, planes and dx read straight off w
            p = torch.arange(B * Hh * W)
            assert torch.equal(c["planes"].permute(0, 2, 3, 1).reshape(-1, 25), c["w"][:, H.onehot_channel(p, cin)].t() + c["b"])
            assert torch.equal(c["dx"].reshape(-1, cin), c["w"][H.onehot_plane(p)])
            assert (c["gn"].sum(3) == 1).all() and c["db"].sum() == B * Hh * W
            if B * Hh * W >= 4 * cin:
                assert len(set(H.onehot_channel(p, cin).tolist())) == cin


def test_k1c_two_trip_case_meets_the_preconditions():
    """The in-process two-trip case at the size a 256-CU part gives it, (1, 260, 512), at the narrowest width."""
    shape = H.two_trip_shape(256)
    assert shape == (1, 260, 512)
    c = H.head_case(shape, 32, "random")
    for dt in H.DTYPES:
        H.preconditions(c, dt)


@pytest.mark.parametrize("shape,C", _K1P, ids=[f"{s}-{c}" for s, c in _K1P])
def test_k1p_cases_meet_the_preconditions(shape, C):
    forms = H.k1p_forms(shape)
    assert forms[0] == "random" and len(forms) >= 2
    for form in forms:
        c = H.head1_case(shape, C, form)
        for dt in H.DTYPES:
            H.preconditions(c, dt)
        assert H.references_agree(c) == 2
        B, Hh, W = shape
        assert c["y"].shape == (B, 1, Hh, W) and c["dx"].shape == (B, Hh, W, C) and c["dW"].shape == (1, C, 3, 3)
        if form != "random":       # the footprint: dx around the point is every channel's flipped kernel
            py, px = (int(v) for v in form[6:].split(","))
            assert c["dW"].sum() == 1 and c["dW"][0, (py + px) % C, 1, 1] == 1 and c["db"].item() == 1
            assert torch.equal(c["dx"][B - 1, py, px], c["w"][0, :, 1, 1])
            if px + 1 < W:
                assert torch.equal(c["dx"][B - 1, py, px + 1], c["w"][0, :, 1, 2])
                assert c["y"][B - 1, 0, py, px + 1] == c["w"][0, (py + px) % C, 1, 0] + 5


def test_the_tables_are_the_ones_the_edges_ask_for():
    assert len(H.K1C_SHAPES) == 6 and all((h * w) % 32 == 0 for _, h, w in H.K1C_SHAPES)
    assert [H.head_trips(b * h * w // 32, H.head_grid_rows(b * h * w // 32, 256)) for b, h, w in H.K1C_SHAPES[:2]] == \
        [[1, 0, 0, 0], [1, 1, 0, 0]]
    # (3, 4, 24): 3 groups per image, so the first workgroup's four waves sit in images 0, 0, 0, 1
    assert [32 * g // 96 for g in range(4)] == [0, 0, 0, 1]
    cs = {C for _, t in H.K1P_TABLE for C in t}
    assert cs == set(H.K1P_CS) and {64 % (C // 8) != 0 for C in (24, 40, 72, 200, 248)} == {True}
    assert {(C // 8) % 4 for C in H.K1P_CS} == {0, 1, 3}                   # the forward's unroll-by-4 remainders
    hs, ws = {s[1] for s, _ in H.K1P_TABLE}, {s[2] for s, _ in H.K1P_TABLE}
    assert {7, 8, 9, 33} <= hs and {63, 64, 65, 255, 256, 257} <= ws
    assert max(H.k1p_tiles(s) for s, t in H.K1P_TABLE if 256 in t) == H.k1p_tiles((1, 33, 65)) == 4
    assert H.delta_points((1, 9, 257)) == [(0, 0), (7, 63), (8, 64), (7, 255), (8, 256)]
    assert H.delta_points((1, 33, 65)) == [(0, 0), (7, 63), (8, 64), (31, 63), (32, 64)]
    assert H.delta_points((1, 1, 1)) == [(0, 0)]


def test_a_broken_case_fails_its_preconditions():
    c = dict(H.head_case((1, 4, 8), 32, "random"))
    c["x"] = c["x"] * 0.5
    with pytest.raises(AssertionError, match="integer"):
        H.preconditions(c, "f32")
    c = dict(H.head_case((1, 4, 8), 32, "random"))
    c["dx"] = c["dx"] * 64
    c["ref64"] = dict(c["ref64"], dx=c["ref64"]["dx"] * 64)
    H.preconditions(c, "f32")
    with pytest.raises(AssertionError, match="stored"):
        H.preconditions(c, "bf16")
    c = dict(H.head1_case((1, 1, 1), 256, "random"))
    c["x"], c["w"] = c["x"] * 64, c["w"] * 64                                  # 9 * 256 * 192 * 192 > 2^24
    with pytest.raises(AssertionError, match="partial sums"):
        H.preconditions(c, "f32")


def test_the_grid_rule():
    assert H.head_groups_per_sweep(256) == 4096 and H.head_groups_per_sweep(304) == 4864
    assert H.head_groups_per_sweep(2048) == 4 * 4096                        # the 4096-workgroup cap
    assert H.head_groups_per_sweep(256, 0) == 4                             # JSPSR_HEAD_WGS=0: one workgroup
    assert H.head_grid_rows(18, 256) == 5 and H.head_grid_rows(18, 256, 0) == 1 and H.head_grid_rows(10 ** 6, 256) == 1024
    assert H.head_trips(18, 1) == [5, 5, 4, 4] and H.head_trips(1, 1) == [1, 0, 0, 0]
    for cus in (64, 256, 304):
        b, h, w = H.two_trip_shape(cus)
        groups = b * h * w // 32
        rows = H.head_grid_rows(groups, cus)
        trips = H.head_trips(groups, rows)
        assert groups == H.head_groups_per_sweep(cus) + 64 and trips.count(2) == 64 and trips.count(1) == 4 * rows - 64
        assert rows <= H.HEAD_MAX_WGS


def _mutant_table():
    lines = [f"{'mutant':<56}{'tensor':<13}{'wrong':>7}  {'exact':<8}{'old f32':<9}{'old bf16':<10}an old case reaches it"]
    for name, (_, reached) in H.MUTANTS.items():
        for what, got, want, view in H.run_mutant(name):
            n = int((got != want).sum())
            assert n > 0, name
            with pytest.raises(AssertionError, match="differ"):
                H.check(got, want, name, view)
            B, Hh, W = H._M_K1C[0] if what.startswith("k1c") else H._M_K1P[0]
            old = []
            for dt in H.DTYPES:
                g = got.bfloat16().float() if (dt == "bf16" and what.endswith(("_dx", "_gn"))) else got
                a = H.old_criteria(g, want, what, dt, B * Hh * W)
                old.append("unseen" if a is None else ("accepts" if a else "rejects"))
            lines.append(f"{name:<56}{what:<13}{n:>7}  {'caught':<8}{old[0]:<9}{old[1]:<10}{reached}")
    return lines


def test_assert_exact_catches_every_mutant():
    """Each planted fault fails the exact comparison.  What the tolerance criteria would have said is printed, not
    asserted: a record of the gap, not a statement about the older tests."""
    lines = _mutant_table()
    print("\n".join(lines))
    assert len(lines) == 1 + len(H.MUTANTS) + 2          # two mutants damage two tensors each
    wanted = ("second-trip", "planes 8 and 9", "halves", "25..31", "halo column", "ky = 0", "inactive-lane", "beside", "fold")
    assert all(any(k in name for name in H.MUTANTS) for k in wanted)


def test_a_mutant_failure_names_the_place():
    what, got, want, view = H.run_mutant("k1c: second-trip group left unwritten")[0]
    with pytest.raises(AssertionError) as e:
        H.check(got, want, "m", view)
    assert "by group in image: {4: " in str(e.value) and "by b: {0: " in str(e.value)
    what, got, want, view = H.run_mutant("k1p: tap ky = 0 dropped at band row y = 8")[0]
    with pytest.raises(AssertionError) as e:
        H.check(got, want, "m", view)
    assert "by y % 32: {8: " in str(e.value) and "by y % 8: {0: " in str(e.value)
    what, got, want, view = H.run_mutant("k1c: dx channel halves swapped")[0]
    with pytest.raises(AssertionError) as e:
        H.check(got, want, "m", view)
    assert "by channel half: {0: " in str(e.value) and ", 1: " in str(e.value)


# ---- K1c's refusals, through ctypes with pointers that are never dereferenced -------------------------------------------
F32, BF16 = 0, 1


def _lib():
    from jspsr_amd import _lib as L
    return L.load()


def _fwd(lib, dtype, B, Hh, W, cin, cs=None, coff=0, x=4096, w=4096, b=4096, planes=4096):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.jspsr_head_forward(dtype, p(x), cin if cs is None else cs, coff, cin, p(w), p(b), p(planes), B, Hh, W, None)


def _bwd(lib, dtype, B, Hh, W, cin, cs=None, coff=0, g=4096, w=4096, dx=4096, gn=4096, db=4096, ws=4096):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.jspsr_head_backward(dtype, p(g), p(w), cin, p(dx), cin if cs is None else cs, coff, p(gn), p(db), p(ws), B, Hh, W, None)


def test_k1c_entry_points_refuse_without_a_gpu():
    lib = _lib()
    err = lambda: lib.jspsr_last_error()
    for entry, name in ((_fwd, b"head_forward"), (_bwd, b"head_backward")):
        for dtype in (F32, BF16):
            assert entry(lib, dtype, 1, 4, 9, 64) == -1 and name in err()              # H W % 32
            assert entry(lib, dtype, 1, 3, 5, 64) == -1 and name in err()
            for cin in (48, 256, 0, 16):
                assert entry(lib, dtype, 1, 4, 8, cin, cs=256) == -1 and name in err(), cin
            assert entry(lib, dtype, 0, 4, 8, 64) == -1 and name in err()              # B = 0
            assert entry(lib, dtype, 1, 4, 8, 64, cs=56) == -1 and name in err()       # pitch < Cin
            assert entry(lib, dtype, 1, 4, 8, 64, cs=72, coff=16) == -1 and b"pitch" in err() and name in err()   # pitch < coff + Cin
            assert entry(lib, dtype, 1, 4, 8, 64, cs=96, coff=-8) == -1 and b"pitch" in err()   # an offset before the tensor
        assert entry(lib, 2, 1, 4, 8, 64) == -1 and name in err()                      # dtype
        assert entry(lib, -1, 1, 4, 8, 64) == -1
        # 16-byte chunks: bf16 pitch / offset in multiples of 8, fp32 of 4
        assert entry(lib, BF16, 1, 4, 8, 64, cs=68) == -1 and b"16-byte" in err() and name in err()
        assert entry(lib, BF16, 1, 4, 8, 64, cs=80, coff=4) == -1 and b"16-byte" in err()
        assert entry(lib, F32, 1, 4, 8, 64, cs=66) == -1 and b"16-byte" in err()
        assert entry(lib, F32, 1, 4, 8, 64, cs=72, coff=2) == -1 and b"16-byte" in err()
    # misalignment is its own code
    assert _fwd(lib, F32, 1, 4, 8, 64, x=4096 + 8) == -2 and b"head_forward" in err() and b"aligned" in err()
    assert _fwd(lib, F32, 1, 4, 8, 64, planes=4096 + 2) == -2 and b"head_forward" in err()
    assert _bwd(lib, BF16, 1, 4, 8, 64, dx=4096 + 8) == -2 and b"head_backward" in err()
    assert _bwd(lib, BF16, 1, 4, 8, 64, gn=4096 + 8) == -2 and b"head_backward" in err()
    assert _bwd(lib, BF16, 1, 4, 8, 64, ws=4096 + 4) == -2 and b"head_backward" in err()
    assert _bwd(lib, F32, 1, 4, 8, 64, g=4096 + 1) == -2 and b"head_backward" in err()
    # null pointers; a null grad_x alone is no refusal reason (it asks for no data gradient), so its pitch is not looked at
    for k in ("x", "w", "b", "planes"):
        assert _fwd(lib, F32, 1, 4, 8, 64, **{k: 0}) == -1 and b"head_forward: null" in err(), k
    for k in ("g", "w", "gn", "db", "ws"):
        assert _bwd(lib, F32, 1, 4, 8, 64, **{k: 0}) == -1 and b"head_backward: null" in err(), k
    assert _bwd(lib, F32, 1, 4, 9, 64, dx=0) == -1 and b"head_backward" in err()
    assert lib.jspsr_head_backward_workspace_bytes(1, 4, 8) == H.HEAD_MAX_WGS * 32 * 4


def test_head_ok_agrees_with_the_forward_entry():
    """jspsr_head_ok(dtype, B, H, W, Cin) is true exactly where jspsr_head_forward on a dense tensor gets as far as the
    launch.  Without a GPU the accepted calls cannot be made, so the agreement is stated from the refusing side: every
    argument set head_ok rejects is refused by the entry with head_ok's name in the message."""
    lib = _lib()
    n = 0
    for dtype in (-1, 0, 1, 2):
        for B in (0, 1, 3):
            for Hh, W in ((4, 8), (4, 9), (0, 32), (32, 0), (1, 32), (3, 5), (32, 5)):
                for cin in (0, 16, 32, 48, 64, 128, 256):
                    want = dtype in (0, 1) and B > 0 and Hh > 0 and W > 0 and (Hh * W) % 32 == 0 and cin in (32, 64, 128)
                    assert bool(lib.jspsr_head_ok(dtype, B, Hh, W, cin)) == want, (dtype, B, Hh, W, cin)
                    if not want:
                        assert _fwd(lib, dtype, B, Hh, W, cin) == -1 and b"jspsr_head_ok" in lib.jspsr_last_error()
                        n += 1
    assert n > 500
