"""Pooled scores over valid pixels (K18) without a GPU: the rank arithmetic the device forms from a count it has just made
(`jspsr_summary_ranks`, the host twin of the kernel's inline) against `summary.segment_ranks`; the host paths of
`pooled_rows` / `scores_pooled` / `summarise(valid=...)` against the restatement on the host-compacted error vector
(tests/summary_ref.py: `scores(e[valid], value_max)`, `check_row`); argument errors in Python and at the C entries before
any launch; header, binding and library; `valid_plane` against `data.void_pixels`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import summary as S
from tests import summary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMAX = 933.0
ENTRIES = {"jspsr_summary_valid_workspace_bytes": 4, "jspsr_summary_valid_forward": 18, "jspsr_summary_ranks": 2}
P = dict(elev_min=-80, elev_max=933, elev_log=True)


# ---- the rank arithmetic ---------------------------------------------------------------------------------------------
def rank_cases():
    rs = np.random.RandomState(18)
    ns = list(range(1, 20001))
    for k in range(1, 33):
        ns += [n for n in range(2 ** k - 3, 2 ** k + 4) if 1 <= n <= 2 ** 32 - 1]
    ns += [int(n) for n in rs.randint(1, 2 ** 32, size=4000, dtype=np.int64)]
    return ns


def test_device_rank_arithmetic_is_segment_ranks():
    lib = _lib.load()
    out = (ctypes.c_longlong * 5)()
    ns = rank_cases()
    assert 2 ** 32 - 1 in ns and 1 in ns
    for n in ns:
        assert lib.jspsr_summary_ranks(n, out) == 0
        m0, m1, l0, l1, g = S.segment_ranks(n)
        assert (out[0], out[1], out[2], out[3]) == (m0, m1, l0, l1), n
        assert out[4] == int(np.float64(g).view(np.int64)), (n, g)                 # bit for bit
    assert lib.jspsr_summary_ranks(0, out) == -1 and b"summary_ranks" in lib.jspsr_last_error()
    assert lib.jspsr_summary_ranks(-3, out) == -1 and lib.jspsr_summary_ranks(5, None) == -1


# ---- host paths ------------------------------------------------------------------------------------------------------
def small_case():
    rs = np.random.RandomState(3)
    gt = rs.uniform(100, 600, (2, 12, 17)).astype(np.float32)
    cands = [(gt + rs.standard_normal(gt.shape) * s).astype(np.float32) for s in (0.5, 6.0)]
    valid = rs.rand(*gt.shape) < 0.6
    segs = [[(0, 1, 2, 9, 13), (1, 0, 0, 12, 17)], [(1, 3, 3, 4, 5)], [(0, 0, 0, 2, 3)]]
    valid[0, 0:2, 0:3] = False                                                    # the last segment is empty
    for c in cands:                                                               # what is masked must not matter
        c[~valid] = -32767.0
    gt[0, 5, 5], valid[0, 5, 5] = np.nan, False
    return gt, cands, valid, segs


def compact(cand, gt, valid, wins):
    e = np.concatenate([(cand[p, y:y + h, x:x + w] - gt[p, y:y + h, x:x + w]).flatten() for p, y, x, h, w in wins]).astype(np.float32)
    v = np.concatenate([valid[p, y:y + h, x:x + w].flatten() for p, y, x, h, w in wins])
    return e[v]


def check_rows(rows, counts, cands, gt, valid, segs, tag):
    assert rows.shape == (len(cands), len(segs), 11) and rows.dtype == np.float32
    assert counts.dtype == np.int64 and counts.shape == (len(segs),)
    for s, wins in enumerate(segs):
        for c, cand in enumerate(cands):
            e = compact(cand, gt, valid, wins)
            assert counts[s] == e.size, (tag, s)
            if e.size == 0:
                assert np.isnan(rows[c, s]).all(), (tag, c, s)
            else:
                R.check_row(rows[c, s], R.scores(e, VMAX), f"{tag} cand {c} seg {s}")


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_scores_pooled_host_path_matches_the_compacted_restatement(dtype):
    gt, cands, valid, segs = small_case()
    v = torch.from_numpy(valid) if dtype == torch.bool else torch.from_numpy(valid.astype(np.uint8) * 7)       # any non-zero byte
    rows, counts = S.scores_pooled([torch.from_numpy(c) for c in cands], torch.from_numpy(gt), segments=segs, value_max=VMAX, valid=v)
    assert counts.tolist()[2] == 0
    check_rows(rows.numpy(), counts.numpy(), cands, gt, valid, segs, "host")
    assert np.isfinite(rows.numpy()[:, :2]).all()


def test_valid_none_is_todays_call():
    gt, cands, valid, segs = small_case()
    gt[0, 5, 5] = 300.0
    t = [torch.from_numpy(c) for c in cands]
    plain = S.scores_pooled(t, torch.from_numpy(gt), segments=segs, value_max=VMAX)
    assert isinstance(plain, torch.Tensor) and plain.shape == (2, 3, 11)
    again = S.scores_pooled(t, torch.from_numpy(gt), segments=segs, value_max=VMAX, valid=None)
    assert isinstance(again, torch.Tensor) and again.numpy().tobytes() == plain.numpy().tobytes()
    ones, counts = S.scores_pooled(t, torch.from_numpy(gt), segments=segs, value_max=VMAX, valid=torch.ones(gt.shape, dtype=torch.bool))
    assert ones.numpy().tobytes() == plain.numpy().tobytes()
    assert counts.tolist() == [sum(w[3] * w[4] for w in wins) for wins in segs]


def cpu_scenes(n_sc=3, full=20, seed=5):
    rs = np.random.RandomState(seed)
    gts = [rs.uniform(150, 400, (full, full)).astype(np.float32) + 37 * i for i in range(n_sc)]
    lrs = [g + rs.uniform(-5, 5, g.shape).astype(np.float32) for g in gts]
    scenes = D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, device="cpu", **P)
    return scenes, gts, lrs, rs


def masked_scores(rasters, gts, valids, b):
    e = np.concatenate([(R.crop(r, b, g.shape) - R.crop(g, b, g.shape))[R.crop(v, b, g.shape) != 0] for r, g, v in zip(rasters, gts, valids)])
    return e.astype(np.float32)


@pytest.mark.parametrize("form", ["list", "flat"])
def test_summarise_host_path_with_valid(form):
    scenes, gts, lrs, rs = cpu_scenes()
    b = 2                                                                         # int(16 * 0.125)
    valids = [rs.rand(20, 20) < 0.7 for _ in gts]
    valids[1][:] = False                                                          # one scene fully masked
    preds = [(g + rs.standard_normal(g.shape)).astype(np.float32) for g in gts]
    for p, v in zip(preds, valids):
        p[~v] = -32767.0
    given = [preds[0], preds[1][b:-b, b:-b].copy(), preds[2]]                     # whole and cropped rasters
    valid = valids if form == "list" else torch.from_numpy(np.concatenate([v.reshape(-1) for v in valids]).astype(np.uint8))
    pooled, means, per = S.summarise(scenes, given, baselines={"COP30": "lr_dem"}, value_max=VMAX, border=0.125, patch_size=16,
                                     online=True, valid=valid)
    for name, rasters in (("SR", preds), ("COP30", lrs)):
        e = masked_scores(rasters, gts, valids, b)
        want = R.scores(e, VMAX)
        assert pooled[name]["N"] == e.size == sum(int(v[b:-b, b:-b].sum()) for v in valids)
        R.check_row(np.array([pooled[name][k] for k in R.COLUMNS] + list(want["brackets"])), want, f"pooled {name}")
        scored = []
        for i, sid in enumerate(scenes.ids):
            e = masked_scores(rasters[i:i + 1], gts[i:i + 1], valids[i:i + 1], b)
            got = per[name][sid]
            assert got["N"] == e.size
            if e.size == 0:
                assert i == 1 and all(np.isnan(got[k]) for k in R.COLUMNS)
                continue
            want = R.scores(e, VMAX)
            R.check_row(np.array([got[k] for k in R.COLUMNS] + list(want["brackets"])), want, f"{name} {sid}")
            scored.append(got)
        for k in R.COLUMNS:
            assert means[name][k] == sum(s[k] for s in scored) / 2
    only = S.summarise(scenes, given, value_max=VMAX, border=0.125, patch_size=16, valid=valid)
    assert only == {"SR": pooled["SR"]}
    plain = S.summarise(scenes, [g.copy() for g in lrs], value_max=VMAX, border=0.125, patch_size=16)
    assert set(plain["SR"]) == set(R.COLUMNS)                                     # no "N" without valid


def test_valid_plane_is_the_complement_of_void_pixels():
    scenes, gts, lrs, rs = cpu_scenes()
    hr = scenes.store["hr_dem"]
    hr[3], hr[17], hr[401], hr[450], hr[900] = -32767.0, float("nan"), float("inf"), float("-inf"), -32767.0
    host = hr.numpy()
    for nodata in (-32767, -32767.0000001, float("nan"), -99999.0):
        plane = S.valid_plane(scenes, nodata)
        assert plane.dtype == torch.uint8 and plane.shape == hr.shape and plane.device == hr.device
        assert np.array_equal(plane.numpy() != 0, ~D.void_pixels(host, nodata)), nodata
    also = torch.from_numpy((rs.rand(hr.numel()) < 0.5))
    both = S.valid_plane(scenes, -32767, also=[also, also.to(torch.uint8)])
    assert np.array_equal(both.numpy() != 0, ~D.void_pixels(host, -32767) & also.numpy())
    assert np.array_equal(S.valid_plane(scenes, -32767, also=also).numpy(), both.numpy())
    with pytest.raises(ValueError, match="also"):
        S.valid_plane(scenes, -32767, also=also[:-1])
    with pytest.raises(ValueError, match="also"):
        S.valid_plane(scenes, -32767, also=also.float())


# ---- argument errors -------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    gt = torch.zeros(64)
    win = [(0, 8, 8, (0, 8), [(0, 8)])]
    ok = torch.ones(64, dtype=torch.uint8)
    rows, counts = S.pooled_rows([gt], gt, win, 1, VMAX, valid=ok)
    assert rows.shape == (1, 1, 11) and counts.tolist() == [64]
    for bad in (ok.bool(), ok.float(), ok[:63], ok.view(8, 8), torch.ones(128, dtype=torch.uint8)[::2], np.ones(64, np.uint8)):
        with pytest.raises(ValueError, match="valid"):
            S.pooled_rows([gt], gt, win, 1, VMAX, valid=bad)
    g2 = gt.view(1, 8, 8)
    for bad in (torch.ones(8, 8, dtype=torch.bool), torch.ones(1, 8, 8), torch.ones(1, 8, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="valid"):
            S.scores_pooled(g2, g2, valid=bad)
    scenes, gts, lrs, rs = cpu_scenes()
    kw = dict(value_max=VMAX, border=0.0, patch_size=16)
    for bad in ([np.ones((20, 20), bool)] * 2, [np.ones((20, 19), bool)] * 3, [np.ones((20, 20), np.float32)] * 3,
                torch.ones(1199, dtype=torch.uint8), torch.ones(1200, dtype=torch.bool)):
        with pytest.raises(ValueError, match="valid"):
            S.summarise(scenes, lrs, valid=bad, **kw)
    with pytest.raises(NotImplementedError, match=r"hr_dem.*summarise\(valid="):
        D.DeviceScenes([lrs[0][..., None]], [gts[0][..., None]], device="cpu", nodata=-32767, **P)


def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL / JSPSR_EALIGN with a message that names the entry, before a launch (safe without a GPU: no device
    pointer is dereferenced, the host arrays are real)."""
    lib = _lib.load()
    x, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    labels = (b"summary_valid_prepare", b"summary_valid_select", b"summary_prepare", b"summary_select")
    before = {n: lib.jspsr_launch_count(n) for n in labels}
    ptrs, numel = (ctypes.c_void_p * 8)(*[4096] * 8), (ctypes.c_longlong * 8)(*[64] * 8)

    def call(cands=ptrs, n_cand=1, gt=x, gt_numel=64, valid=x, valid_numel=64, windows=x, n_windows=1, segments=x, n_segments=1,
             total=64, chunks=1, out=x, counts=x, ws=x):
        return lib.jspsr_summary_valid_forward(cands, numel, n_cand, gt, gt_numel, valid, valid_numel, windows, n_windows, segments,
                                               n_segments, total, chunks, VMAX, out, counts, ws, None)

    def message():
        return lib.jspsr_last_error().decode()

    for kw in (dict(cands=None), dict(gt=None), dict(valid=None), dict(counts=None), dict(windows=None), dict(segments=None),
               dict(out=None), dict(ws=None), dict(n_cand=0), dict(n_cand=9), dict(n_windows=0), dict(total=0), dict(gt_numel=0),
               dict(valid_numel=63), dict(valid_numel=65), dict(total=2 ** 32, chunks=2 ** 19), dict(chunks=3), dict(n_segments=2)):
        assert call(**kw) == -1 and "summary_valid_forward" in message(), kw
    assert call(valid_numel=63) == -1 and "validity plane" in message()
    nulls = (ctypes.c_void_p * 8)(4096, None, *[4096] * 6)
    assert call(cands=nulls, n_cand=2) == -1 and "candidate 1" in message()
    for kw in (dict(gt=odd), dict(out=odd), dict(ws=ctypes.c_void_p(4104)), dict(counts=ctypes.c_void_p(4100))):
        assert call(**kw) == -2 and "aligned" in message() and "summary_valid_forward" in message(), kw
    size, plain = lib.jspsr_summary_valid_workspace_bytes, lib.jspsr_summary_workspace_bytes
    assert size(0, 1, 64, 1) == 0 and size(1, 1, 2 ** 32, 2 ** 19) == 0 and size(9, 1, 64, 1) == 0
    for args in ((1, 1, 64, 1), (3, 5, 100000, 17), (8, 1, 4096 * 4096, 2048)):
        extra = size(*args) - plain(*args)                                        # a byte per element, a word per chunk, rounded up
        assert plain(*args) > 0 and args[2] + 4 * args[3] <= extra <= args[2] + 4 * args[3] + 32, args
    assert before == {n: lib.jspsr_launch_count(n) for n in labels}


def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert "K18 (ABI v25, additive)" in hdr
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\b(?:int|size_t)\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    lib.jspsr_abi_version.restype = ctypes.c_int
    assert lib.jspsr_abi_version() == 25 == _lib.load().jspsr_abi_version()
    k12 = re.search(r"\bint\s+jspsr_summary_forward\s*\((.*?)\);", hdr, re.S).group(1)
    assert len(k12.split(",")) == len(_lib.SIGNATURES["jspsr_summary_forward"][1]) == 15          # the unmasked entry is untouched
    assert all(callable(getattr(S, name)) for name in ("valid_plane", "pooled_rows", "scores_pooled", "summarise"))
