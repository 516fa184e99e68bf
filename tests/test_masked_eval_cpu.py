"""Masked per-tile meters (K20) without a GPU: the numpy restatement (tests/masked_eval_ref.py) pinned by construction to
tests/eval_ref.py (all-ones plane: equal; rectangular valid region: the cropped tile); `evaluate._scores_torch(valid=)`
and a CPU `PerformanceMeter(masked=True)` against it; argument errors in Python and at the C entries before any launch;
header, binding and library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import evaluate as EV
from jspsr_amd import metrics as M
from tests import eval_ref as E
from tests import masked_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"jspsr_scores_batch_valid_workspace_bytes": 3, "jspsr_scores_batch_valid_forward": 14}
GARBAGE = (float("nan"), float("inf"), -float("inf"), -32767.0, 1e30)


def tiles(n, H, W, seed):
    """(pred, gt) fp32 (n,1,H,W) in the network's range: smooth fields plus noise, an exact-zero patch (ties)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64) / max(H, W)
    gt = 0.5 + 0.15 * np.sin(5.0 * xx + 0.3)[None] * np.cos(4.0 * yy)[None] + rs.normal(0.0, 0.002, (n, H, W))
    pred = gt + rs.normal(0.0003, 0.002, (n, H, W))
    pred[:, 4:7, 3:9] = gt[:, 4:7, 3:9]
    return pred[:, None].astype(np.float32), gt[:, None].astype(np.float32)


def speckle(n, H, W, void, seed):
    return (np.random.RandomState(seed).rand(n, 1, H, W) >= void).astype(np.uint8)


def poison(a, valid, shift=0):
    """`a` with GARBAGE cycling through its masked places."""
    out = a.copy()
    idx = np.flatnonzero(valid.ravel() == 0)
    out.ravel()[idx] = np.array(GARBAGE, dtype=np.float32)[(np.arange(idx.size) + shift) % len(GARBAGE)]
    return out


# ---- the restatement is eval_ref's by construction ---------------------------------------------------------------------
@pytest.mark.parametrize("border,lg", [(0.0, True), (0.05, True), (0.05, False)])
def test_restatement_with_all_ones_is_eval_ref(border, lg):
    pred, gt = tiles(2, 40, 52, seed=1)
    ones = np.ones_like(pred, dtype=np.uint8)
    got, counts = R.batch_scores(pred, gt, ones, E.VMIN, E.VMAX, border, lg)
    want = E.batch_scores(pred, gt, E.VMIN, E.VMAX, border, lg)
    assert np.array_equal(got, want), np.abs(got - want).max(0)
    h, w = 40 - 2 * int(40 * border), 52 - 2 * int(52 * border)
    assert counts.tolist() == [[h * w, (h - 2) * (w - 2), h * w]] * 2


@pytest.mark.parametrize("border,rect", [(0.0, (3, 30, 5, 41)), (0.05, (6, 25, 9, 30)), (0.0, (10, 13, 20, 23))])
def test_restatement_with_a_rectangle_is_eval_ref_of_the_cropped_tile(border, rect):
    y0, y1, x0, x1 = rect                      # strictly inside the crop, in uncropped coordinates
    pred, gt = tiles(2, 40, 52, seed=2)
    valid = np.zeros_like(pred, dtype=np.uint8)
    valid[..., y0:y1, x0:x1] = 1
    pred_g, gt_g = poison(pred, valid), poison(gt, valid, 2)
    hh, ww = y1 - y0, x1 - x0
    for lg in (True, False):
        got, counts = R.batch_scores(pred_g, gt_g, valid, E.VMIN, E.VMAX, border, lg)
        want = E.batch_scores(pred[..., y0:y1, x0:x1], gt[..., y0:y1, x0:x1], E.VMIN, E.VMAX, 0.0, lg)
        assert np.allclose(got[:, :7], want[:, :7], rtol=1e-12, atol=0), (got - want)[:, :7]
        # column 7 differs by design at the rectangle's rim (a clamped tap there is a void, not a replica): its count instead
        assert counts.tolist() == [[hh * ww, (hh - 2) * (ww - 2), (hh - 2) * (ww - 2)]] * 2
        assert np.isfinite(got[:, 7]).all()


def test_restatement_zero_counts_are_nan():
    pred, gt = tiles(1, 12, 12, seed=3)
    void = np.zeros((12, 12), np.uint8)
    s, c = R.tile_scores(pred[0, 0], gt[0, 0], void, E.VMIN, E.VMAX, 0.0, True)
    assert np.isnan(s).all() and c.tolist() == [0, 0, 0]
    yy, xx = np.mgrid[0:12, 0:12]
    s, c = R.tile_scores(pred[0, 0], gt[0, 0], ((yy + xx) % 2).astype(np.uint8), E.VMIN, E.VMAX, 0.0, True)
    assert np.isfinite(s[:6]).all() and np.isnan(s[6:]).all() and c.tolist() == [72, 0, 0]


# ---- the torch route of the meter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("border,lg", [(0.0, True), (0.05, False)])
def test_scores_torch_valid_against_the_restatement(border, lg):
    pred, gt = tiles(4, 37, 53, seed=4)
    valid = speckle(4, 37, 53, 0.2, seed=5)
    valid[1] = 0                                                  # a fully void tile
    valid[2, 0] = (np.add.outer(np.arange(37), np.arange(53)) % 2).astype(np.uint8)     # a checkerboard: no slope
    valid[3, 0, :, 26:] = 0                                       # a half plane
    want, wc = R.batch_scores(pred, gt, valid, E.VMIN, E.VMAX, border, lg)
    args = (torch.from_numpy(poison(pred, valid)), torch.from_numpy(poison(gt, valid, 3)), E.VMIN, E.VMAX, border, lg)
    got, gc = EV._scores_torch(*args, valid=torch.from_numpy(valid))
    assert got.dtype == torch.float32 and gc.dtype == torch.int32 and np.array_equal(gc.numpy(), wc)
    got = got.numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[1]).all() and np.isnan(got[2, 6:]).all() and np.isfinite(got[2, :6]).all() and np.isfinite(got[0]).all()
    ok = ~np.isnan(want)
    tol = np.where(np.arange(8) < 2, 1e-3, 2e-3 + 1e-5 * np.abs(np.nan_to_num(want)))
    assert np.all((np.abs(got - want) <= tol)[ok]), np.abs(got - want)
    # a bool plane is the same call; all-ones is the unmasked route
    again, ac = EV._scores_torch(*args, valid=torch.from_numpy(valid).bool())
    assert np.array_equal(again.numpy(), got.astype(np.float32), equal_nan=True) and torch.equal(ac, gc)
    clean = (torch.from_numpy(pred), torch.from_numpy(gt), E.VMIN, E.VMAX, border, lg)
    ones, oc = EV._scores_torch(*clean, valid=torch.ones(pred.shape, dtype=torch.uint8))
    plain = EV._scores_torch(*clean)
    assert torch.allclose(ones, plain, rtol=1e-5, atol=1e-5) and torch.equal(ones[:, 3:6], plain[:, 3:6])
    h, w = 37 - 2 * int(37 * border), 53 - 2 * int(53 * border)
    assert oc.tolist() == [[h * w, (h - 2) * (w - 2), h * w]] * 4
    for bad in (torch.ones(4, 1, 37, 52, dtype=torch.uint8), torch.ones(pred.shape), valid):
        with pytest.raises(ValueError, match="valid"):
            EV._scores_torch(*clean, valid=bad)


CFG = {"PSNR": {"package": "local"}, "RMSE": {"package": "local"}, "Median": {}, "NMAD": {}, "LE95": {},
       "Slope": {"package": "local"}}


def meter_case():
    pred, gt = tiles(5, 24, 24, seed=6)
    valid = speckle(5, 24, 24, 0.1, seed=7)
    valid[1] = 0                                                                         # fully void
    valid[3, 0] = (np.add.outer(np.arange(24), np.arange(24)) % 2).astype(np.uint8)      # checkerboard
    return pred, gt, valid


def test_cpu_masked_meter_scores_counts_worst_and_clone():
    pred, gt, valid = meter_case()
    want, wc = R.batch_scores(pred, gt, valid, E.VMIN, E.VMAX, 0.0, True)
    meter = EV.PerformanceMeter(CFG, E.VMIN, E.VMAX, border=0.0, elev_log=True, masked=True)
    p, g, v = torch.from_numpy(poison(pred, valid)), torch.from_numpy(poison(gt, valid, 1)), torch.from_numpy(valid)
    meter.update(p[:2], g[:2], meta=[{"id": "a"}, {"id": "b"}], valid=v[:2])
    meter.update(p[2:], g[2:], meta=[{"id": "c"}, {"id": "d"}, {"id": "e"}], valid=v[2:].bool())
    assert len(meter) == 5
    counts = meter.counts()
    assert counts.dtype == np.int32 and counts.shape == (5, 3) and np.array_equal(counts, wc)
    assert counts[1].tolist() == [0, 0, 0] and counts[3].tolist() == [288, 0, 0]
    table, meta = meter.table()
    assert table.shape == (5, 6) and np.isnan(table[1]).all() and np.isnan(table[3, 5]) and np.isfinite(table[3, :5]).all()
    scores = meter.get_score()
    assert list(scores) == list(CFG)
    cols = (1, 2, 3, 4, 5, 6)
    for j, (name, col) in enumerate(zip(CFG, cols)):
        keep = [i for i in range(5) if wc[i, M.COUNT_OF_COLUMN[col]] > 0]
        assert keep == ([0, 2, 4] if name == "Slope" else [0, 2, 3, 4])              # per-column exclusion
        ref = sum(want[i, col] for i in keep) / len(keep)
        assert math.isfinite(scores[name]) and abs(scores[name] - ref) <= 2e-3 + 1e-5 * abs(ref), (name, scores[name], ref)
        assert scores[name] == sum(float(table[i, j]) for i in keep) / len(keep)
    # worst() skips the NaN row; the walk over the rest is eval_ref's
    rm = [float(x) for x in table[:, 1]]
    finite = [(i, x) for i, x in zip("abcde", rm) if x == x]
    assert len(finite) == 4
    assert meter.worst("RMSE") == [(finite[j][0], finite[j][1]) for j, _ in E.worst([x for _, x in finite])]
    # clone keeps the flag, reset empties the counts
    twin = meter.clone()
    assert twin.masked and len(twin) == 0 and twin.counts().shape == (0, 3)
    twin.update(p[:1], g[:1])                                                             # valid=None: every pixel, full counts
    assert twin.counts().tolist() == [[576, 484, 576]]
    plain = EV.PerformanceMeter(CFG, E.VMIN, E.VMAX, border=0.0, elev_log=True)
    plain.update(torch.from_numpy(pred[:1]), torch.from_numpy(gt[:1]))
    twin.reset()
    twin.update(torch.from_numpy(pred[:1]), torch.from_numpy(gt[:1]))
    assert np.allclose(twin.table()[0], plain.table()[0], rtol=1e-5, atol=1e-5)
    assert not plain.masked and not plain.clone().masked
    meter.reset()
    assert len(meter) == 0 and meter.counts().shape == (0, 3)
    with pytest.raises(ValueError, match="no sample"):
        meter.get_score()


def test_masked_meter_refusals():
    pred, gt, valid = meter_case()
    p, g, v = torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(valid)
    for package in ("piq", "local"):
        with pytest.raises(NotImplementedError, match="SSIM"):
            EV.PerformanceMeter({"RMSE": {}, "SSIM": {"package": package}}, E.VMIN, E.VMAX, masked=True)
    EV.PerformanceMeter({"RMSE": {}, "SSIM": {"package": "piq"}}, E.VMIN, E.VMAX)          # unmasked: as before
    plain = EV.PerformanceMeter(CFG, E.VMIN, E.VMAX, border=0.0)
    with pytest.raises(ValueError, match="masked=True"):
        plain.update(p, g, valid=v)
    assert len(plain) == 0
    with pytest.raises(ValueError, match="masked=True"):
        plain.counts()
    meter = EV.PerformanceMeter(CFG, E.VMIN, E.VMAX, border=0.0, masked=True)
    for bad in (v[:, :, :23], v.float(), v[:4], valid):
        with pytest.raises(ValueError, match="valid"):
            meter.update(p, g, valid=bad)
    assert len(meter) == 0
    # a metric no tile has a valid pixel for is named
    meter.update(p[3:4], g[3:4], valid=v[3:4])                                             # the checkerboard: no slope
    with pytest.raises(ValueError, match="Slope"):
        meter.get_score()
    only = EV.PerformanceMeter({"RMSE": {}}, E.VMIN, E.VMAX, border=0.0, masked=True)
    only.update(p[1:2], g[1:2], valid=v[1:2])                                              # fully void
    with pytest.raises(ValueError, match="RMSE"):
        only.get_score()
    assert only.worst("RMSE") == []


class Half(torch.nn.Module):
    def forward(self, lr):
        return lr * 0.5 + 0.25


class Crit:
    """The smallest criterion `evaluate` accepts: masked L1, one sample at a time."""

    def reset(self):
        pass

    def __call__(self, pred, gt, valid=None):
        d = (pred - gt).abs()
        v = torch.ones_like(d, dtype=torch.bool) if valid is None else valid != 0
        l1 = torch.where(v, d, torch.zeros_like(d)).sum() / v.sum().clamp(min=1)
        return {"L1": l1, "Total": l1}


def test_evaluate_passes_the_plane_to_both_meters_cpu():
    pred, gt, valid = meter_case()
    lr = torch.from_numpy(poison(pred, valid * 0 + 1))
    batches = [{"lr_dem": lr[lo:hi], "hr_dem": torch.from_numpy(poison(gt, valid))[lo:hi], "base": None,
                "meta": [{"id": i} for i in range(lo, hi)], "valid": torch.from_numpy(valid)[lo:hi]} for lo, hi in ((0, 3), (3, 5))]
    meter = EV.PerformanceMeter(CFG, E.VMIN, E.VMAX, border=0.0, elev_log=True, masked=True)
    scores, total, terms, scores_in = EV.evaluate(Half(), batches, Crit(), meter, "JSPSR", {"lr_dem": 1}, compare_input=True)
    want_in, wc = R.batch_scores(pred, gt, valid, E.VMIN, E.VMAX, 0.0, True)
    want, _ = R.batch_scores(pred * 0.5 + 0.25, gt, valid, E.VMIN, E.VMAX, 0.0, True)
    assert np.array_equal(meter.counts(), wc) and math.isfinite(total)
    for got, ref in ((scores, want), (scores_in, want_in)):
        for name, col in zip(CFG, (1, 2, 3, 4, 5, 6)):
            keep = wc[:, M.COUNT_OF_COLUMN[col]] > 0
            r = ref[keep, col].mean()
            assert abs(got[name] - r) <= 2e-3 + 1e-5 * abs(r), (name, got[name], r)
    plain = EV.PerformanceMeter(CFG, E.VMIN, E.VMAX, border=0.0, elev_log=True)
    with pytest.raises(NotImplementedError, match=r"meter.*masked=True"):
        EV.evaluate(Half(), batches, Crit(), plain, "JSPSR", {"lr_dem": 1})


# ---- the C entries -----------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN with a message that names the entry, before a launch (safe without a GPU: no device
    pointer is dereferenced)."""
    lib = _lib.load()
    x, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    labels = (b"scores_batch_valid (lds)", b"scores_batch_valid (stream)", b"scores_batch (lds)", b"scores_batch (stream)")
    before = {n: lib.jspsr_launch_count(n) for n in labels}

    def call(pred=x, gt=x, valid=x, B=2, H=32, W=32, border=0.0, vmin=0.0, vmax=2.0, out=x, counts=x, ws=x):
        return lib.jspsr_scores_batch_valid_forward(pred, gt, valid, B, H, W, border, vmin, vmax, 0, out, counts, ws, None)

    def message():
        return lib.jspsr_last_error().decode()

    for kw in (dict(pred=None), dict(gt=None), dict(valid=None), dict(counts=None), dict(out=None), dict(ws=None), dict(B=0), dict(B=-3),
               dict(H=0), dict(W=0), dict(border=0.5), dict(border=-0.1), dict(border=float("nan")), dict(vmax=1.0),
               dict(vmin=5.0, vmax=5.5), dict(H=2), dict(W=2), dict(H=20, W=4, border=0.45), dict(H=40000, W=40000),
               dict(B=65536, H=160, W=160)):
        assert call(**kw) == -1 and "scores_batch_valid_forward" in message(), kw
    assert call(valid=None) == -1 and "validity plane" in message()
    for kw in (dict(pred=odd), dict(gt=odd), dict(out=odd), dict(counts=odd), dict(ws=ctypes.c_void_p(4104))):
        assert call(**kw) == -2 and "aligned" in message() and "scores_batch_valid_forward" in message(), kw
    assert call(valid=ctypes.c_void_p(4097), B=0) == -1                                   # the plane needs no alignment
    size, plain = lib.jspsr_scores_batch_valid_workspace_bytes, lib.jspsr_scores_batch_workspace_bytes
    assert size(0, 32, 32) == 0 and size(2, 0, 32) == 0 and size(2, 32, -1) == 0
    assert size(5, 128, 128) == plain(5, 128, 128) == 16 == size(5, 142, 142)             # LDS path: nothing is staged
    for B, H, W in ((1, 143, 142), (5, 160, 150), (8, 512, 512)):
        blocks = min(1024, -(-H * W // 2048))
        assert plain(B, H, W) > 0 and 0 <= size(B, H, W) - plain(B, H, W) - 16 * B * blocks < 16, (B, H, W)
    lib.jspsr_scores_batch_forward.restype = ctypes.c_int
    assert lib.jspsr_scores_batch_forward(x, x, 0, 32, 32, 0.0, 0.0, 2.0, 0, x, x, None) == -1
    assert "scores_batch_forward" in message() and "valid" not in message()               # the unmasked entry keeps its name
    assert before == {n: lib.jspsr_launch_count(n) for n in labels}


def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert "K20 (ABI v25, additive)" in hdr
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\b(?:int|size_t)\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    lib.jspsr_abi_version.restype = ctypes.c_int
    assert lib.jspsr_abi_version() == 25 == _lib.load().jspsr_abi_version()
    k10 = re.search(r"\bint\s+jspsr_scores_batch_forward\s*\((.*?)\);", hdr, re.S).group(1)
    assert len(k10.split(",")) == len(_lib.SIGNATURES["jspsr_scores_batch_forward"][1]) == 12      # the unmasked entry is untouched
    assert M.COUNT_COLUMNS == ("N", "N_slope_local", "N_slope_kornia") and len(M.COUNT_OF_COLUMN) == len(M.SCORE_COLUMNS)


def test_python_argument_errors_need_no_gpu():
    pred, gt, valid = meter_case()
    with pytest.raises(ValueError):                                                        # CPU tensors: refused before the plane is looked at
        M.batch_scores(torch.from_numpy(pred), torch.from_numpy(gt), 0.0, 2.0, valid=torch.from_numpy(valid))
