"""SSIM over a validity plane (K23, the "window" rule) without a GPU: the restatement tests/masked_ssim_ref.py against the
unmasked restatements it must reduce to (tests/loss_menu_ref.py), its counts, its gradient, the rectangle identity; the CPU
path and the host logic of `PerformanceMeter(masked=True, ssim_valid="window")`; the keyword's refusals; header, binding
and library; the new entries' argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import evaluate as EV
from jspsr_amd import losses as L
from jspsr_amd import metrics as MT
from tests import loss_menu_ref as M
from tests import masked_ssim_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"jspsr_loss_menu_valid_ssim_workspace_bytes": 5, "jspsr_loss_menu_valid_ssim_forward": 15,
           "jspsr_loss_menu_valid_ssim_backward": 13, "jspsr_ssim_tiles_workspace_bytes": 5, "jspsr_ssim_tiles_forward": 13}


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.SHAPES)
def test_all_ones_plane_is_the_unmasked_restatement(shape):
    p, g = (t.double() for t in S.pair(shape))
    ones = np.ones(shape, bool)
    vals, grad, n = S.values_and_grad({"ssim": 1.0}, p, g, ones)
    v64, g64 = M.value_and_grad(M.ssim_loss, p, g)
    assert n == shape[0] * shape[1] * (shape[2] - 10) * (shape[3] - 10)
    assert rel(vals["ssim"], v64) <= 1e-12 and rel(vals["Total"], v64) <= 1e-12
    assert (grad - g64).abs().max().item() <= 1e-12 * g64.abs().max().item()
    # the per-tile forms, both packages
    w = MT.local_window()
    x = p.clamp(0, 1)
    for b in range(shape[0]):
        piq, n_piq = S.tiles(p[b:b + 1, :1], g[b:b + 1, :1], None, "piq")
        assert rel(piq[0], M.ssim_piq(x[b:b + 1, :1], g[b:b + 1, :1]).item()) <= 1e-12 and n_piq[0] == (shape[2] - 10) * (shape[3] - 10)
        loc, n_loc = S.tiles(p[b:b + 1, :1], g[b:b + 1, :1], ones[b:b + 1, :1], "local", window=w)
        assert rel(loc[0], M.ssim_local(x[b:b + 1, :1], g[b:b + 1, :1], w.double()).item()) <= 1e-12 and n_loc[0] == shape[2] * shape[3]


def counts(shape, name, same=False):
    v = S.expand(S.planes(shape)[name], torch.empty(shape))
    return S.counted_map(v, same).sum((1, 2, 3)).tolist()


def test_counted_maps_match_the_rule():
    a, b = (2, 1, 23, 37), (1, 2, 45, 76)
    assert counts(a, "ones") == [351, 351]
    assert counts(a, "pixel") == [230, 230] and counts(a, "corner") == [350, 350] and counts(a, "rect") == [327, 327]
    assert counts(a, "island") == [1, 0] and counts(a, "sample") == [0, 345] and counts(a, "none") == [0, 0]
    assert counts(a, "pixel", True) == [730, 730] and counts(a, "corner", True) == [815, 815] and counts(a, "rect", True) == [732, 732]
    assert counts(a, "ones", True) == [851, 851]
    assert counts(b, "pixel") == [2 * 2189] and counts(b, "rect") == [2 * 2264] and counts(b, "ones") == [2 * 2310]
    assert 300 < counts(b, "speckle")[0] // 2 < 2310
    assert counts((1, 1, 11, 11), "ones") == [1] and counts((1, 1, 11, 11), "pixel") == [0]
    assert counts((3, 1, 43, 54), "island") == [1, 0, 0]
    # the count of the whole call, as values_and_grad reports it
    p, g = S.pair(a)
    assert S.values_and_grad({"ssim": 1.0}, p, g, S.planes(a)["sample"])[2] == 345


def test_gradcheck_in_fp64():
    shape = (1, 1, 13, 14)
    p, g = (t.double() for t in S.pair(shape))
    p = p.clamp(0.05, 0.95)                                  # away from the clamp's kinks
    v = torch.ones(shape, dtype=torch.bool)
    v[0, 0, 1, 12] = False                                   # under the windows of map rows 0..1, columns 2..3: 8 of 12 are left
    assert int(S.counted_map(v).sum()) == 8
    x = torch.where(v, p, torch.zeros_like(p)).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: S.ssim_loss(t, g, v), (x,), eps=1e-6, atol=1e-6)
    _, grad, _ = S.values_and_grad({"ssim": 1.0}, p, g, v)
    assert (grad[~v] == 0).all() and grad.abs().max() > 0


def test_masked_pixels_have_no_influence_and_nothing_counted_is_zero():
    shape = (2, 1, 23, 37)
    p, g = S.pair(shape)
    for name in ("pixel", "rect", "sample"):
        v = S.planes(shape)[name]
        want = S.values_and_grad({"L1": 1, "SSIM": 0.5}, p, g, v)
        for junk in (float("nan"), float("inf"), -32767.0, 1e30):
            p2, g2 = p.clone(), g.clone()
            p2[torch.from_numpy(~v)], g2[torch.from_numpy(~v)] = junk, -junk
            got = S.values_and_grad({"L1": 1, "SSIM": 0.5}, p2, g2, v)
            assert got[0] == want[0] and torch.equal(got[1], want[1]) and got[2] == want[2]
    vals, grad, n = S.values_and_grad({"SSIM": 1.0}, p, g, S.planes(shape)["none"])
    assert n == 0 and vals == {"SSIM": 0.0, "Total": 0.0} and not grad.any()
    t, c = S.tiles(p, g, S.planes(shape)["island"], "piq")
    assert c.tolist() == [1, 0] and np.isfinite(t[0]) and np.isnan(t[1])


def test_rectangle_plane_is_the_unmasked_call_on_the_crop_in_valid_mode():
    """A plane valid exactly on a rectangle of at least 11 x 11: the counted windows are those inside the rectangle, so the
    valid-mode result is the unmasked one on the cropped tensors.  NOT so in same mode: there the crop's border windows
    read zero PADDING, which is not void, while the rectangle's border windows inside the plane read voids and do not
    count -- the masked same-mode map keeps only the windows that lie wholly inside the rectangle."""
    shape = (2, 1, 23, 37)
    p, g = (t.double() for t in S.pair(shape))
    y0, y1, x0, x1 = 3, 19, 5, 30
    v = np.zeros(shape, bool)
    v[..., y0:y1, x0:x1] = True
    vals, grad, n = S.values_and_grad({"ssim": 1.0}, p, g, v)
    v64, g64 = M.value_and_grad(M.ssim_loss, p[..., y0:y1, x0:x1], g[..., y0:y1, x0:x1])
    assert n == 2 * (y1 - y0 - 10) * (x1 - x0 - 10)
    assert rel(vals["ssim"], v64) <= 1e-12
    assert (grad[..., y0:y1, x0:x1] - g64).abs().max().item() <= 1e-12 * g64.abs().max().item()
    inside = torch.zeros(shape, dtype=torch.bool)
    inside[..., y0:y1, x0:x1] = True
    assert (grad[~inside] == 0).all()
    w = MT.local_window()
    masked, cm = S.tiles(p, g, v, "local", window=w)
    cropped, cc = S.tiles(p[..., y0:y1, x0:x1], g[..., y0:y1, x0:x1], None, "local", window=w)
    assert cm.tolist() == [(y1 - y0 - 10) * (x1 - x0 - 10)] * 2 and cc.tolist() == [(y1 - y0) * (x1 - x0)] * 2
    assert abs(masked[0] - cropped[0]) > 1e-6


# ---- the CPU meter path and the host logic -----------------------------------------------------------------------------
METRICS = {"RMSE": {"package": "local"}, "SSIM": {"package": "piq"}, "ssim": {"package": "local"}}


def meter(**kw):
    return EV.PerformanceMeter(METRICS, 0.0, 2.0, border=0.05, elev_log=False, **kw)


def test_cpu_meter_against_the_restatement():
    B, H, W = 4, 40, 44
    p, g = S.pair((B, 1, H, W))
    rs = np.random.RandomState(3)
    v = rs.rand(B, 1, H, W) >= 0.004
    v[1] = False                                             # a void tile
    v[2] = True
    v[3, 0, :, :20] = False                                  # leaves windows on the right only
    m = meter(masked=True, ssim_valid="window")
    assert m.count_names == list(MT.COUNT_COLUMNS) + ["N_SSIM", "N_ssim"] and tuple(MT.COUNT_COLUMNS) == ("N", "N_slope_local", "N_slope_kornia")
    p2 = p.clone()
    p2[torch.from_numpy(~v)] = float("nan")
    m.update(p2[:3], g[:3], valid=torch.from_numpy(v[:3]))
    m.update(p2[3:], g[3:], valid=torch.from_numpy(v[3:]).to(torch.uint8) * 3)
    table, _ = m.table()
    cnt = m.counts()
    assert table.shape == (4, 3) and cnt.shape == (4, 5) and cnt.dtype == np.int32
    for j, package in ((1, "piq"), (2, "local")):
        want, wc = S.tiles(p, g, v, package, 0.05, window=MT.local_window(), dtype=torch.float32)
        want64, _ = S.tiles(p, g, v, package, 0.05, window=MT.local_window())
        assert cnt[:, 2 + j].tolist() == wc.tolist() and wc[1] == 0 and wc[0] > 0 and wc[3] > 0
        assert wc[2] == ((36 - 10) * (40 - 10) if package == "piq" else 36 * 40)
        assert np.isnan(table[1, j]) and np.isnan(want[1])
        keep = [0, 2, 3]
        assert np.abs(table[keep, j] - want64[keep]).max() <= 4 * np.abs(want[keep] - want64[keep]).max() + 1e-6
    assert np.isnan(table[1, 0]) and cnt[1].tolist() == [0] * 5
    score = m.get_score()
    assert list(score) == list(METRICS)
    for j, k in enumerate(METRICS):
        assert score[k] == sum(float(x) for x in table[[0, 2, 3], j]) / 3
    # an all-ones plane: the unmasked meter's values
    ones = meter(masked=True, ssim_valid="window")
    ones.update(p, g)
    plain = meter()
    plain.update(p, g)
    assert np.allclose(ones.table()[0], plain.table()[0], rtol=1e-6, atol=1e-7)
    # worst() skips the NaN row; clone() carries the keyword
    assert m.worst("SSIM", 4) == []                          # three tiles with a value: the reference ranks more than three only
    m.update(p[:2], g[:2])
    worst = m.worst("ssim", 2)
    assert len(m) == 6 and len(worst) == 2 and all(i != 1 and v == v for i, v in worst)
    c = m.clone()
    assert c.ssim_valid == "window" and c.masked and c.count_names == m.count_names and len(c) == 0
    # no tile with a counted element: get_score names the metric
    none = meter(masked=True, ssim_valid="window")
    half = torch.ones(1, 1, H, W, dtype=torch.bool)
    half[..., ::6, ::6] = False
    none.update(p[:1], g[:1], valid=half)
    with pytest.raises(ValueError, match="SSIM"):
        none.get_score()
    assert none.counts()[0, 0] > 0 and none.counts()[0, 3] == 0 and none.counts()[0, 4] == 0


def test_keyword_refusals_and_defaults():
    with pytest.raises(ValueError, match="ssim_valid"):
        meter(ssim_valid="window")                           # without masked=True
    with pytest.raises(ValueError, match="ssim_valid"):
        meter(masked=True, ssim_valid="renormalised")
    with pytest.raises(NotImplementedError, match="SSIM"):
        meter(masked=True)                                   # the default still refuses
    for make in (lambda **kw: L.get_loss("ssim", **kw), lambda **kw: L.get_criterion({"L1": 1, "SSIM": 0.5}, **kw),
                 lambda **kw: L.Criterion({"SSIM": 1.0}, **kw), lambda **kw: L.LossTerm("ssim", **kw)):
        with pytest.raises(ValueError, match="ssim_valid"):
            make(ssim_valid="partial")
        with pytest.raises(ValueError, match="ssim_valid"):
            make(ssim_valid=1)
        assert make(ssim_valid="window").spec.ssim_valid == "window" and make().spec.ssim_valid is None
    assert L.get_criterion({"SSIM": 3.0}, ssim_valid="window").single
    assert L.get_criterion({"L1": 1, "L2": 1}, ssim_valid="window").spec.terms == 0      # accepted where there is no SSIM


# ---- header, binding, library ------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\b(?:int|size_t)\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    assert _lib.load().jspsr_abi_version() == 25
    for entry, n in (("jspsr_loss_menu_valid_forward", 14), ("jspsr_loss_menu_valid_backward", 12), ("jspsr_ssim_forward", 10)):
        proto = re.search(r"\bint\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n, entry      # the existing entries are untouched


def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL before a launch (safe without a GPU: no device pointer is dereferenced)."""
    lib = _lib.load()
    x = ctypes.c_void_p(4096)
    labels = (b"ssim_valid_forward", b"ssim_valid_backward", b"loss_menu_valid_max", b"loss_menu_valid_sum", b"loss_menu_valid_combine",
              b"loss_menu_valid_backward", b"ssim_tiles_forward", b"ssim_tiles_finalize")
    before = {n: lib.jspsr_launch_count(n) for n in labels}
    slots, w, sw = (ctypes.c_int * 1)(6), (ctypes.c_double * 1)(1.0), (ctypes.c_double * 7)(*[1.0] * 7)
    fwd, bwd = lib.jspsr_loss_menu_valid_ssim_forward, lib.jspsr_loss_menu_valid_ssim_backward
    assert fwd(x, x, None, 8, 1, 32, 32, 1, 1, slots, w, None, x, x, None) == -1                 # a null plane
    assert b"loss_menu_valid_ssim_forward" in lib.jspsr_last_error()
    assert fwd(x, x, x, 8, 1, 32, 32, 0, 1, slots, w, None, x, x, None) == -1                    # ssim_rule 0
    assert b"ssim_rule" in lib.jspsr_last_error()
    assert fwd(x, x, x, 8, 1, 32, 32, 2, 1, slots, w, None, x, x, None) == -1
    assert fwd(x, x, x, 8, 1, 10, 32, 1, 1, slots, w, None, x, x, None) == -1                    # H < 11
    assert b"H, W >= 11" in lib.jspsr_last_error()
    assert fwd(x, x, x, 9, 1, 32, 10, 1, 1, slots, w, None, x, x, None) == -1
    assert fwd(x, x, x, 1, 1, 32, 32, 1, 1, slots, w, None, x, x, None) == -1                    # slot 6 is not among terms = BerHu
    assert b"slot 6" in lib.jspsr_last_error()
    assert fwd(x, x, x, 8, 1, 32, 32, 1, 1, (ctypes.c_int * 1)(0), w, None, x, x, None) == -1    # slot 0 without base losses
    assert fwd(x, x, x, 16, 1, 32, 32, 1, 1, slots, w, None, x, x, None) == -1 and fwd(x, x, x, 8, 0, 32, 32, 1, 1, slots, w, None, x, x, None) == -1
    assert bwd(x, x, None, 8, 1, 32, 32, 1, sw, None, x, x, None) == -1
    assert bwd(x, x, x, 8, 1, 32, 32, 0, sw, None, x, x, None) == -1 and b"ssim_rule" in lib.jspsr_last_error()
    assert bwd(x, x, x, 8, 1, 32, 10, 1, sw, None, x, x, None) == -1 and bwd(x, x, x, 8, 1, 32, 32, 1, None, None, x, x, None) == -1
    q = lib.jspsr_loss_menu_valid_ssim_workspace_bytes
    assert q(8, 1, 32, 32, 0) == 0 and q(8, 1, 10, 32, 1) == 0 and q(0, 1, 32, 32, 1) == 0 and q(16, 1, 32, 32, 1) == 0
    assert q(7, 2, 32, 32, 1) == lib.jspsr_loss_menu_valid_workspace_bytes(7, 2, 32, 32) > 0     # without the bit: K19's layout
    assert q(8, 2, 32, 32, 1) >= q(7, 2, 32, 32, 1) + 2 * 22 * 22 * 3 * 4 + 16
    assert q(7, 1, 8, 8, 1) > 0                                                                   # H < 11 matters to SSIM only
    assert lib.jspsr_loss_menu_valid_workspace_bytes(8, 1, 32, 32) == 0                           # the K19 entries still refuse the bit
    assert lib.jspsr_loss_menu_valid_forward(x, x, x, 8, 1, 32, 32, 1, slots, w, None, x, x, None) == -1
    tiles, tq = lib.jspsr_ssim_tiles_forward, lib.jspsr_ssim_tiles_workspace_bytes
    assert tiles(None, x, x, 2, 64, 64, 0.05, 0, None, x, x, x, None) == -1 and b"ssim_tiles_forward" in lib.jspsr_last_error()
    assert tiles(x, x, x, 2, 64, 64, 0.05, 0, None, None, x, x, None) == -1 and tiles(x, x, x, 2, 64, 64, 0.05, 0, None, x, None, x, None) == -1
    assert tiles(x, x, x, 2, 64, 64, 0.05, 0, None, x, x, None, None) == -1 and tiles(x, x, x, 0, 64, 64, 0.05, 0, None, x, x, x, None) == -1
    assert tiles(x, x, x, 2, 64, 64, 0.5, 0, None, x, x, x, None) == -1 and tiles(x, x, x, 2, 64, 64, -0.1, 0, None, x, x, x, None) == -1
    assert tiles(x, x, x, 2, 64, 64, float("nan"), 0, None, x, x, x, None) == -1
    assert tiles(x, x, None, 2, 12, 64, 0.1, 0, None, x, x, x, None) == -1 and b">= 11" in lib.jspsr_last_error()     # 12 - 2 = 10 rows left
    assert tq(2, 64, 64, 0.05, 0) == 2 * 16 * 2 and tq(2, 64, 64, 0.05, 1) == 2 * 16 * 2 and tq(1, 10, 10, 0.0, 1) == 32
    assert tq(2, 64, 64, 0.5, 0) == 0 and tq(0, 64, 64, 0.0, 0) == 0 and tq(1, 10, 64, 0.0, 0) == 0 and tq(1, 12, 64, 0.1, 0) == 0
    assert before == {n: lib.jspsr_launch_count(n) for n in labels}
