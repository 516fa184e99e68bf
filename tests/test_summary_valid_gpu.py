"""K18 on the MI355X: pooled scores over valid pixels (jspsr_summary_valid_forward) against the numpy restatement of
summarise_evaluation on the host-compacted error vector, `summary_ref.scores(e[valid], value_max)`, with the project's K12
tolerances (tests/summary_ref.py: check_row -- the six bracketing order statistics equal as values, Median bit-equal,
NMAD / LE95 / PSNR within 1 fp32 ulp of the float64 value, RMSE within 2 for the order of the sum).

The counts are compared with ==; an all-ones plane, the splits of a call and a second run with `tobytes()`.

One valid NaN: the five scores are NaN, the median and LE95 brackets are the restatement's (np.sort puts the NaN last).
The restatement's MAD brackets are NaN themselves there (np.median of a vector with a NaN), so nothing equals them; the MAD
brackets are checked against the order statistics of |e - m| with m the mean of the two middle elements of np.sort(e),
which is what the row's Median column is made of."""
import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import summary as S
from tests import summary_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VMAX = 933.0
PREPARE, SELECT = b"summary_prepare", b"summary_select"
V_PREPARE, V_SELECT = b"summary_valid_prepare", b"summary_valid_select"


def launches(*names):
    return sum(_lib.load().jspsr_launch_count(n) for n in names)


def pooled(cands, gt, valid, segments=None):
    """numpy (planes, H, W) arrays and a bool plane of gt's shape -> ((n_cand, n_seg, 11) rows, (n_seg,) counts) from the device."""
    cands = [cands] if isinstance(cands, np.ndarray) else cands
    rows, counts = S.scores_pooled([torch.from_numpy(c).to(DEV) for c in cands], torch.from_numpy(gt).to(DEV), segments=segments,
                                   value_max=VMAX, valid=torch.from_numpy(valid).to(DEV))
    assert counts.dtype == torch.int64 and counts.device == rows.device
    return rows.cpu().numpy(), counts.cpu().numpy()


def unmasked(cands, gt, segments=None):
    cands = [cands] if isinstance(cands, np.ndarray) else cands
    return S.scores_pooled([torch.from_numpy(c).to(DEV) for c in cands], torch.from_numpy(gt).to(DEV), segments=segments,
                           value_max=VMAX).cpu().numpy()


def compact(cand, gt, valid, wins=None):
    """The host route: the errors of a segment's windows, then boolean indexing."""
    if wins is None:
        wins = [(p, 0, 0) + gt.shape[1:] for p in range(gt.shape[0])]
    with np.errstate(all="ignore"):
        e = np.concatenate([(cand[p, y:y + h, x:x + w] - gt[p, y:y + h, x:x + w]).flatten() for p, y, x, h, w in wins]).astype(np.float32)
    v = np.concatenate([valid[p, y:y + h, x:x + w].flatten() for p, y, x, h, w in wins])
    return e[v]


def check(rows, counts, cands, gt, valid, segments=None, tag=""):
    cands = [cands] if isinstance(cands, np.ndarray) else cands
    segments = [None] if segments is None else segments
    assert rows.shape == (len(cands), len(segments), 11) and counts.shape == (len(segments),)
    for s, wins in enumerate(segments):
        for c, cand in enumerate(cands):
            e = compact(cand, gt, valid, wins)
            assert counts[s] == e.size, (tag, s, counts[s], e.size)
            if e.size == 0:
                assert np.isnan(rows[c, s]).all(), (tag, c, s, rows[c, s])
            else:
                R.check_row(rows[c, s], R.scores(e, VMAX), f"{tag} cand {c} seg {s} n_v {e.size}")


def errors_case(name):
    """The error sets of tests/test_summary_gpu.py (the ground truth is 0, so e is the candidate itself), as (1, h, w) arrays."""
    rs = np.random.RandomState(len(name))
    if name == "quantised":            # 1/128 steps: heavy ties, zeros, both signs
        e = rs.randint(-5, 6, (1, 61, 67)) / 128.0
    elif name == "all_equal":
        e = np.full((1, 33, 35), -0.375)
    elif name == "wide":               # 1e-6 .. 1e3 in both signs: every digit pass matters
        e = 10.0 ** rs.uniform(-6, 3, (1, 90, 101)) * rs.choice([-1.0, 1.0], (1, 90, 101))
    elif name == "one_top_digit":      # every key of e and |e| shares its top byte: the aggregated increment
        e = rs.uniform(1.0, 1.999, (1, 70, 73))
    elif name == "chunks":             # 25 500 elements: 3 whole chunks of 8192 and one of 924
        e = rs.standard_normal((1, 150, 170)) * 2.5
    elif name == "replicated":         # 1.1e6 elements = 135 chunks: the histograms are spread over 4 replicas
        e = rs.standard_normal((1, 1100, 1000)) * 4.0
    else:
        raise KeyError(name)
    return e.astype(np.float32)


# ---- selection against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_valid", [0, 1, 2, 3])
def test_tiny_counts(n_valid):
    cand = np.array([0.75, -1.5, 0.125, 7.0, -3.0], dtype=np.float32).reshape(1, 1, 5)
    valid = np.zeros((1, 1, 5), bool)
    valid[0, 0, [4, 1, 2][:n_valid]] = True
    rows, counts = pooled(cand, np.zeros_like(cand), valid)
    assert counts.tolist() == [n_valid]
    check(rows, counts, cand, np.zeros_like(cand), valid, tag=f"n_v={n_valid}")


def chunk_mask(kind):
    n, chunk = 150 * 170, S.CHUNK
    assert (n + chunk - 1) // chunk == 4 and n % chunk
    rs = np.random.RandomState(len(kind))
    v = np.ones(n, bool)
    if kind == "void_chunk":
        v[chunk:2 * chunk] = False
    elif kind == "last_chunk_only":
        v[:3 * chunk] = False
        v[3 * chunk:] = rs.rand(n - 3 * chunk) < 0.5
    elif kind == "one_per_chunk":
        v[:] = False
        v[[0, 2 * chunk - 1, 2 * chunk + 4097, n - 1]] = True
    else:
        v = rs.rand(n) < float(kind)
    return v.reshape(1, 150, 170)


@pytest.mark.parametrize("kind", ["void_chunk", "last_chunk_only", "one_per_chunk", "0.99", "0.5", "0.01"])
def test_chunk_boundaries(kind):
    e = errors_case("chunks")
    valid = chunk_mask(kind)
    rows, counts = pooled(e, np.zeros_like(e), valid)
    assert counts[0] == valid.sum() > 0
    check(rows, counts, e, np.zeros_like(e), valid, tag=kind)


@pytest.mark.parametrize("kind", ["random30", "half_plane"])
def test_replicas(kind):
    e = errors_case("replicated")
    if kind == "random30":
        valid = np.random.RandomState(30).rand(*e.shape) >= 0.3
    else:
        valid = np.zeros(e.shape, bool)
        valid[:, :, 500:] = True
    rows, counts = pooled(e, np.zeros_like(e), valid)
    check(rows, counts, e, np.zeros_like(e), valid, tag=kind)


def pitched_case():
    """The windows of tests/test_summary_gpu.py: pitched_case (an odd and an even segment, crops that do not start at 0; plane 0
    rows 10..14, columns 20..28 belong to both), and a mask in the ground truth's layout that flips both parities."""
    rs = np.random.RandomState(7)
    gt = rs.uniform(100, 600, (3, 40, 56)).astype(np.float32)
    cands = [(gt + rs.standard_normal(gt.shape) * s).astype(np.float32) for s in (0.5, 3.0, 0.01, 40.0)]
    odd = [(0, 3, 3, 34, 50), (1, 0, 0, 40, 56), (2, 5, 7, 11, 13)]          # 1700 + 2240 + 143 = 4083
    even = [(2, 1, 2, 37, 53), (0, 10, 20, 5, 9)]                            # 1961 + 45 = 2006
    valid = rs.rand(*gt.shape) < 0.7

    def n_valid(wins):
        return sum(int(valid[p, y:y + h, x:x + w].sum()) for p, y, x, h, w in wins)

    if n_valid(odd) % 2 == 1:
        valid[1, 0, 0] ^= True                                               # a pixel of the odd segment alone
    if n_valid(even) % 2 == 0:
        valid[2, 1, 2] ^= True                                               # a pixel of the even segment alone
    assert n_valid(odd) % 2 == 0 and n_valid(even) % 2 == 1
    shared = valid[0, 10:15, 20:29]
    assert shared.any() and not shared.all()
    return gt, cands, odd, even, valid


def test_pooled_windows_with_pitched_crops():
    gt, cands, odd, even, valid = pitched_case()
    for c in cands:
        c[~valid] = -32767.0
    rows, counts = pooled(cands[:2], gt, valid, [odd, even])
    assert counts[0] % 2 == 0 and counts[1] % 2 == 1
    check(rows, counts, cands[:2], gt, valid, [odd, even], tag="pitched")


@pytest.mark.parametrize("name", ["quantised", "all_equal", "wide", "one_top_digit"])
def test_ties_and_digits(name):
    e = errors_case(name)
    valid = np.random.RandomState(40).rand(*e.shape) >= 0.4
    rows, counts = pooled(e, np.zeros_like(e), valid)
    check(rows, counts, e, np.zeros_like(e), valid, tag=name)


# ---- what is masked has no influence ---------------------------------------------------------------------------------
def poison_case():
    rs = np.random.RandomState(66)
    gt = rs.uniform(100, 600, (1, 97, 103)).astype(np.float32)                  # 9991 elements: two chunks
    cand = (gt + rs.standard_normal(gt.shape) * 2.0).astype(np.float32)
    valid = rs.rand(*gt.shape) < 0.5
    poison = np.array([np.nan, np.inf, -np.inf, -32767.0, 1e30], dtype=np.float32)
    idx = np.flatnonzero(~valid.reshape(-1))
    cand.reshape(-1)[idx] = poison[np.arange(idx.size) % 5]
    gt.reshape(-1)[idx] = poison[(np.arange(idx.size) // 5) % 5]                # every pair of poisons meets
    return gt, cand, valid


def test_masked_poison_has_no_influence():
    gt, cand, valid = poison_case()
    rows, counts = pooled(cand, gt, valid)
    assert np.isfinite(rows).all()
    check(rows, counts, cand, gt, valid, tag="poison")
    clean_c, clean_g = np.where(valid, cand, 0).astype(np.float32), np.where(valid, gt, 0).astype(np.float32)
    again, c2 = pooled(clean_c, clean_g, valid)
    assert again.tobytes() == rows.tobytes() and c2.tolist() == counts.tolist()


def test_one_valid_nan_makes_the_scores_nan_and_keeps_the_brackets():
    gt, cand, valid = poison_case()
    at = np.flatnonzero(valid.reshape(-1))[1234]
    cand.reshape(-1)[at] = np.nan
    rows, counts = pooled(cand, gt, valid)
    e = compact(cand, gt, valid)
    assert counts[0] == e.size and np.isnan(e).sum() == 1
    row = rows[0, 0]
    assert np.isnan(row[:5]).all()
    want = R.scores(e, VMAX)["brackets"]
    assert np.array_equal(row[[5, 6, 9, 10]], want[[0, 1, 4, 5]]) and np.isfinite(row[5:]).all()
    m0, m1, _, _ = R.ranks(e.size)
    srt = np.sort(e)
    with np.errstate(all="ignore"):
        dev = np.sort(np.abs(e - (srt[m0] + srt[m1]) * np.float32(0.5)))
    assert np.array_equal(row[7:9], dev[[m0, m1]])


# ---- an all-ones plane is the unmasked call --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chunks", "wide", "replicated", "pitched"])
def test_all_ones_plane_has_the_unmasked_bits(name):
    if name == "pitched":
        gt, cands, odd, even, _ = pitched_case()
        cands, segs = cands[:2], [odd, even]
        sizes = [4083, 2006]
    else:
        e = errors_case(name)
        gt, cands, segs, sizes = np.zeros_like(e), [e], None, [e.size]
    rows, counts = pooled(cands, gt, np.ones(gt.shape, bool), segs)
    assert rows.tobytes() == unmasked(cands, gt, segs).tobytes()
    assert counts.tolist() == sizes


# ---- independence, determinism, census -------------------------------------------------------------------------------
def twelve_segments():
    rs = np.random.RandomState(12)
    gt = rs.uniform(100, 600, (4, 48, 52)).astype(np.float32)
    cands = [(gt + np.round(rs.standard_normal(gt.shape) * s * 128) / 128).astype(np.float32) for s in (0.3, 2.0, 11.0, 0.02)]
    segs = [[(i % 4, i, i, 20 + i, 25 + i)] + ([(3 - i % 4, 0, 0, 3 + i, 7)] if i % 3 else []) for i in range(12)]
    valid = rs.rand(*gt.shape) < 0.6
    return gt, cands, segs, valid


def test_rows_do_not_depend_on_the_rest_of_the_call():
    gt, cands, segs, valid = twelve_segments()
    plain = launches(PREPARE, SELECT)
    before = launches(V_PREPARE, V_SELECT)
    one, one_n = pooled(cands[:1], gt, valid, segs[:1])
    per_small = launches(V_PREPARE, V_SELECT) - before
    before = launches(V_PREPARE, V_SELECT)
    prepares = launches(V_PREPARE)
    full, full_n = pooled(cands, gt, valid, segs)
    per_full = launches(V_PREPARE, V_SELECT) - before
    assert per_small == per_full == 16 and launches(V_PREPARE) == prepares + 1   # the launch count depends on nothing
    assert launches(PREPARE, SELECT) == plain                                   # the unmasked labels did not move
    assert full.shape == (4, 12, 11) and one.tobytes() == full[:1, :1].tobytes() and one_n.tolist() == full_n[:1].tolist()
    again, again_n = pooled(cands, gt, valid, segs)                              # two runs
    assert again.tobytes() == full.tobytes() and again_n.tolist() == full_n.tolist()
    for c in range(4):                                                           # four candidates = four one-candidate calls
        r, n = pooled(cands[c:c + 1], gt, valid, segs)
        assert r.tobytes() == full[c:c + 1].tobytes() and n.tolist() == full_n.tolist(), c
    for s in range(12):                                                          # twelve segments = twelve one-segment calls
        r, n = pooled(cands, gt, valid, segs[s:s + 1])
        assert r.tobytes() == full[:, s:s + 1].tobytes() and n.tolist() == full_n[s:s + 1].tolist(), s
    check(full[[0, 3]][:, [0, 5, 11]], full_n[[0, 5, 11]], [cands[0], cands[3]], gt, valid, [segs[0], segs[5], segs[11]], tag="twelve")
    assert launches(PREPARE, SELECT) == plain


# ---- summarise(valid=...) --------------------------------------------------------------------------------------------
def test_summarise_over_valid_pixels_online():
    n_sc, full, b = 5, 70, 1                                                     # b = int(32 * 0.05)
    rs = np.random.RandomState(18)
    gts = [rs.uniform(150, 400, (full, full)).astype(np.float32) + 37 * i for i in range(n_sc)]
    lrs = [g + rs.uniform(-5, 5, g.shape).astype(np.float32) for g in gts]
    scenes = D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, elev_min=-80,
                            elev_max=933, elev_log=True, device=DEV)
    valids = [rs.rand(full, full) < 0.8 for _ in range(n_sc)]
    valids[3][:] = False                                                         # one scene fully masked
    preds = [(g + rs.standard_normal(g.shape) * 1.5).astype(np.float32) for g in gts]
    for p, v in zip(preds, valids):
        p[~v] = -32767.0                                                         # as predict_scenes(mask_voids=True) leaves them
    given = [p if i % 2 else p[b:-b, b:-b].copy() for i, p in enumerate(preds)]  # cropped and whole rasters
    flat = torch.from_numpy(np.concatenate([v.reshape(-1) for v in valids]).astype(np.uint8)).to(DEV)
    kw = dict(baselines={"COP30": "lr_dem"}, value_max=VMAX, border=0.05, patch_size=32, online=True)
    before, plain = launches(V_PREPARE, V_SELECT), launches(PREPARE, SELECT)
    got = S.summarise(scenes, given, valid=valids, **kw)
    assert launches(V_PREPARE, V_SELECT) == before + 16 and launches(PREPARE, SELECT) == plain
    assert _nan_to_none(S.summarise(scenes, given, valid=flat, **kw)) == _nan_to_none(got)      # the mask as a flat device tensor
    pooled_, means, per_scene = got

    def errors(rasters, idx):
        return np.concatenate([(R.crop(rasters[i], b, gts[i].shape) - R.crop(gts[i], b, gts[i].shape))[valids[i][b:-b, b:-b].reshape(-1)]
                               for i in idx]).astype(np.float32)

    for name, rasters in (("SR", preds), ("COP30", lrs)):
        e = errors(rasters, range(n_sc))
        want = R.scores(e, VMAX)
        assert pooled_[name]["N"] == e.size
        R.check_row(np.array([pooled_[name][k] for k in R.COLUMNS] + list(want["brackets"])), want, f"offline {name}")
        scored = []
        for i, sid in enumerate(scenes.ids):
            e = errors(rasters, [i])
            row = per_scene[name][sid]
            assert row["N"] == e.size
            if i == 3:
                assert e.size == 0 and all(np.isnan(row[k]) for k in R.COLUMNS)
                continue
            want = R.scores(e, VMAX)
            R.check_row(np.array([row[k] for k in R.COLUMNS] + list(want["brackets"])), want, f"online {name} {sid}")
            scored.append(row)
        for k in R.COLUMNS:
            assert means[name][k] == sum(r[k] for r in scored) / (n_sc - 1)


def _nan_to_none(tree):
    """Dicts / tuples of floats with NaN replaced by None, so that == compares them."""
    if isinstance(tree, dict):
        return {k: _nan_to_none(v) for k, v in tree.items()}
    if isinstance(tree, (tuple, list)):
        return tuple(_nan_to_none(v) for v in tree)
    return None if isinstance(tree, float) and tree != tree else tree
