"""K12 on the MI355X: the pooled selection (jspsr_summary_forward) against the numpy restatement of summarise_evaluation
(tests/summary_ref.py), its independence of the other rows of a call, determinism and launch census; the scene assembly
(jspsr_scenes_assemble_f32) against the composition the package runs scene by scene; `evaluate(..., collector=)` end to
end; and the entry's error codes.

Tolerances (tests/summary_ref.py: check_row): the six bracketing order statistics equal as values, Median bit-equal,
NMAD / LE95 / PSNR within 1 fp32 ulp of the float64 value (one final rounding gives <= 0.5), RMSE within 2 (sum order)."""
import ctypes

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import evaluate as EV
from jspsr_amd import losses as L
from jspsr_amd import summary as S
from tests import batches_ref as B
from tests import summary_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VMAX = 933.0
PREPARE, SELECT, ASSEMBLE = b"summary_prepare", b"summary_select", b"scenes_assemble"


def launches(*names):
    return sum(_lib.load().jspsr_launch_count(n) for n in names)


def pooled(cands, gt, segments=None):
    """numpy (planes, H, W) arrays -> (n_cand, n_seg, 11) numpy rows from the device."""
    cands = [cands] if isinstance(cands, np.ndarray) else cands
    rows = S.scores_pooled([torch.from_numpy(c).to(DEV) for c in cands], torch.from_numpy(gt).to(DEV), segments=segments, value_max=VMAX)
    return rows.cpu().numpy()


def segment_errors(cand, gt, wins):
    return np.concatenate([(cand[p, y:y + h, x:x + w] - gt[p, y:y + h, x:x + w]).flatten() for p, y, x, h, w in wins]).astype(np.float32)


def errors_case(name):
    """Error vectors (the ground truth is 0, so e is the candidate itself), as (1, h, w) arrays."""
    rs = np.random.RandomState(len(name))
    if name == "quantised":            # 1/128 steps: heavy ties, zeros, both signs
        e = rs.randint(-5, 6, (1, 61, 67)) / 128.0
    elif name == "all_equal":
        e = np.full((1, 33, 35), -0.375)
    elif name == "wide":               # 1e-6 .. 1e3 in both signs: every digit pass matters
        e = 10.0 ** rs.uniform(-6, 3, (1, 90, 101)) * rs.choice([-1.0, 1.0], (1, 90, 101))
    elif name == "one_top_digit":      # every key of e and |e| shares its top byte: the aggregated increment
        e = rs.uniform(1.0, 1.999, (1, 70, 73))
    elif name == "large":              # ~3e5 elements: many chunks per segment, the grid-stride boundaries
        e = rs.standard_normal((1, 512, 600)) * 2.5
    elif name == "replicated":         # 1.1e6 elements = 135 chunks: the histograms are spread over 4 replicas
        e = rs.standard_normal((1, 1100, 1000)) * 4.0
    else:
        raise KeyError(name)
    return e.astype(np.float32)


# ---- selection against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_segments(n):
    cand = np.array([0.75, -1.5, 0.125], dtype=np.float32)[:n].reshape(1, 1, n)
    gt = np.zeros_like(cand)
    R.check_row(pooled(cand, gt)[0, 0], R.scores(cand.flatten(), VMAX), f"n={n}")


@pytest.mark.parametrize("name", ["quantised", "all_equal", "wide", "one_top_digit", "large", "replicated"])
def test_selection_matches_restatement(name):
    e = errors_case(name)
    rows = pooled(e, np.zeros_like(e))
    R.check_row(rows[0, 0], R.scores(e.flatten(), VMAX), name)


def pitched_case():
    rs = np.random.RandomState(7)
    gt = rs.uniform(100, 600, (3, 40, 56)).astype(np.float32)
    cands = [(gt + rs.standard_normal(gt.shape) * s).astype(np.float32) for s in (0.5, 3.0, 0.01, 40.0)]
    odd = [(0, 3, 3, 34, 50), (1, 0, 0, 40, 56), (2, 5, 7, 11, 13)]          # 1700 + 2240 + 143 = 4083
    even = [(2, 1, 2, 37, 53), (0, 10, 20, 5, 9)]                            # 1961 + 45 = 2006
    return gt, cands, odd, even


def test_pooled_windows_with_pitched_crops():
    gt, cands, odd, even = pitched_case()
    assert sum(w[3] * w[4] for w in odd) % 2 == 1 and sum(w[3] * w[4] for w in even) % 2 == 0
    rows = pooled(cands[:2], gt, [odd, even])
    for c in range(2):
        for s, wins in enumerate((odd, even)):
            R.check_row(rows[c, s], R.scores(segment_errors(cands[c], gt, wins), VMAX), f"cand {c} seg {s}")


def test_nan_and_zero_error_rows():
    gt = np.random.RandomState(1).uniform(0, 9, (2, 30, 31)).astype(np.float32)
    cand = gt.copy()
    cand[1] += 1.0
    cand[1, 7, 9] = np.nan
    rows = pooled(cand, gt, [[(0, 0, 0, 30, 31)], [(1, 0, 0, 30, 31)]])
    assert rows[0, 0, 4] == np.inf and (rows[0, 0, :4] == 0).all()
    assert np.isnan(rows[0, 1, :5]).all()


# ---- independence, determinism, census -------------------------------------------------------------------------------
def twelve_segments():
    rs = np.random.RandomState(12)
    gt = rs.uniform(100, 600, (4, 48, 52)).astype(np.float32)
    cands = [(gt + np.round(rs.standard_normal(gt.shape) * s * 128) / 128).astype(np.float32) for s in (0.3, 2.0, 11.0, 0.02)]
    segs = [[(i % 4, i, i, 20 + i, 25 + i)] +([(3 - i % 4, 0, 0, 3 + i, 7)] if i % 3 else []) for i in range(12)]
    return gt, cands, segs


def test_rows_do_not_depend_on_the_rest_of_the_call():
    gt, cands, segs = twelve_segments()
    lib_before = launches(PREPARE, SELECT)
    one = pooled(cands[:1], gt, segs[:1])
    per_small = launches(PREPARE, SELECT) - lib_before
    lib_before = launches(PREPARE, SELECT)
    full = pooled(cands, gt, segs)
    per_full = launches(PREPARE, SELECT) - lib_before
    assert per_small == per_full == 16                                   # the launch count depends on nothing
    assert full.shape == (4, 12, 11) and one.tobytes() == full[:1, :1].tobytes()
    assert pooled(cands, gt, segs).tobytes() == full.tobytes()            # two runs
    for c in range(4):                                                    # four candidates = four one-candidate calls
        assert pooled(cands[c:c + 1], gt, segs).tobytes() == full[c:c + 1].tobytes(), c
    for s in range(12):                                                   # twelve segments = twelve one-segment calls
        assert pooled(cands, gt, segs[s:s + 1]).tobytes() == full[:, s:s + 1].tobytes(), s
    for c in (0, 3):
        for s in (0, 5, 11):
            R.check_row(full[c, s], R.scores(segment_errors(cands[c], gt, segs[s]), VMAX), f"cand {c} seg {s}")


# ---- assembly --------------------------------------------------------------------------------------------------------
def square_scenes(n_sc, full, lg, seed):
    rs = np.random.RandomState(seed)
    gts = [rs.uniform(150, 400, (full, full)).astype(np.float32) + 37 * i for i in range(n_sc)]
    lrs = [g + rs.uniform(-5, 5, g.shape).astype(np.float32) for g in gts]                   # distinct bases (relative)
    return D.DeviceScenes(lr_dem=[a[..., None] for a in lrs], hr_dem=[a[..., None] for a in gts], relative=True, elev_min=-80,
                          elev_max=933, elev_log=lg, device=DEV)


@pytest.mark.parametrize("full,k,n,border", [(70, 32, 9, 0.05), (70, 32, 9, 0.0), (48, 32, 4, 0.1), (32, 32, 1, 0.05)])
@pytest.mark.parametrize("n_sc", [1, 5])
@pytest.mark.parametrize("lg", [True, False])
def test_assembly_is_the_composition_in_one_launch(full, k, n, border, n_sc, lg):
    scenes = square_scenes(n_sc, full, lg, seed=full + n + n_sc)
    assert len({float(b) for b in scenes.base}) == n_sc
    tiles = torch.from_numpy(np.random.RandomState(5).uniform(-0.2, 1.2, (n_sc * n, 1, k, k)).astype(np.float32)).to(DEV)
    c = S.ScenePredictions(scenes, k, n, border=border)
    before = launches(ASSEMBLE)
    c.add(tiles, [{"id": scenes.ids[i // n]} for i in range(n_sc * n)])
    assert launches(ASSEMBLE) == before + 1
    got = c.rasters()
    for i, sid in enumerate(scenes.ids):
        want = R.assemble(tiles[i * n:(i + 1) * n], scenes.base[i], full, border, -80, 933, lg).cpu().numpy()
        assert got[sid].shape == want.shape
        assert got[sid].tobytes() == want.tobytes(), (sid, np.abs(got[sid] - want).max())


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_evaluate_with_a_collector_end_to_end():
    from jspsr_amd.JSPSR import Model
    ic = {"lr_dem": 1, "image": 3}
    raw = B.make_scenes([(70, 70)] * 3, seed=31)
    kinds = {k: [s[k] for s in raw] for k in ("lr_dem", "hr_dem", "image")}
    scenes = D.DeviceScenes(**kinds, device=DEV, relative=True, elev_min=-80, elev_max=933, elev_log=True)
    torch.manual_seed(0)
    model = Model(dict(ic, COP30=1), num_feature=8).to(DEV).eval()
    metric = {"RMSE": {"package": "local"}, "Median": {"package": "local"}}

    def run(collector):
        meter = EV.PerformanceMeter(metric, -80, 933, border=0.05, elev_log=True)
        batches = D.TileCropBatches(scenes, 10, 32, 9)                    # 27 tiles in batches of 10: scenes straddle them
        return EV.evaluate(model, batches, L.get_criterion({"L1": 1, "L2": 1}), meter, "JSPSR", ic, collector=collector)

    c = S.ScenePredictions(scenes, 32, 9, border=0.05)

    class Recorder:                                                       # the tile predictions the collector was handed
        seen = []

        def add(self, pred, meta):
            self.seen.append(pred.clone())
            c.add(pred, meta)

    with_c, without = run(Recorder()), run(None)
    assert with_c == without                                              # the collector changes nothing evaluate returns
    assert c.complete and [p.shape[0] for p in Recorder.seen] == [10, 10, 7]
    rasters = c.rasters()
    preds = torch.cat(Recorder.seen)
    for i, sid in enumerate(scenes.ids):
        want = R.assemble(preds[9 * i:9 * i + 9], scenes.base[i], 70, 0.05, -80, 933, True).cpu().numpy()
        assert rasters[sid].shape == (68, 68) and rasters[sid].tobytes() == want.tobytes(), sid
    before = launches(PREPARE, SELECT)
    got, means, per_scene = S.summarise(scenes, c, baselines={"COP30": "lr_dem"}, value_max=VMAX, border=0.05, patch_size=32, online=True)
    assert launches(PREPARE, SELECT) == before + 16
    gts = [s["hr_dem"][..., 0] for s in raw]
    off, onl, per = R.summarise(gts, {"SR": [rasters[s] for s in scenes.ids], "COP30": [s["lr_dem"][..., 0] for s in raw]}, 1, VMAX)
    for name in ("SR", "COP30"):
        R.check_row(np.array([got[name][k] for k in R.COLUMNS] + list(off[name]["brackets"])), off[name], f"offline {name}")
        for i, sid in enumerate(scenes.ids):
            R.check_row(np.array([per_scene[name][sid][k] for k in R.COLUMNS] + list(per[name][i]["brackets"])), per[name][i],
                        f"online {name} {sid}")
        for k in R.COLUMNS:
            assert means[name][k] == sum(per_scene[name][s][k] for s in scenes.ids) / 3


# ---- error codes -----------------------------------------------------------------------------------------------------
def test_bad_arguments_give_error_codes_and_no_launch():
    lib = _lib.load()
    x = torch.zeros(64, device=DEV)
    n_win, n_seg, total, chunks = 1, 1, 64, 1
    tab = torch.zeros(n_win * 22 + n_seg * 8, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.jspsr_summary_workspace_bytes(1, 1, total, chunks) + 16, dtype=torch.uint8, device=DEV)
    assert ws.numel() > 16 and ws.data_ptr() % 16 == 0
    out = torch.empty(11, device=DEV)
    ptrs, numel = (ctypes.c_void_p * 9)(*[x.data_ptr()] * 9), (ctypes.c_longlong * 9)(*[64] * 9)

    def call(cands=ptrs, n_cand=1, gt=x.data_ptr(), windows=tab.data_ptr(), n_windows=n_win, tot=total, o=out.data_ptr(), w=ws.data_ptr()):
        return lib.jspsr_summary_forward(cands, numel, n_cand, gt, 64, windows, n_windows, tab.data_ptr() + 22 * 8, n_seg, tot, chunks, VMAX,
                                         o, w, torch.cuda.current_stream().cuda_stream)

    before = launches(PREPARE, SELECT)
    EINVAL, EALIGN = -1, -2                                              # include/jspsr_hip.h
    assert call(cands=None) == EINVAL and call(gt=None) == EINVAL and call(windows=None) == EINVAL
    assert call(o=None) == EINVAL and call(w=None) == EINVAL
    assert call(n_cand=0) == EINVAL and call(n_cand=9) == EINVAL
    assert call(n_windows=0) == EINVAL and call(tot=0) == EINVAL          # an empty table
    assert call(w=ws.data_ptr() + 4) == EALIGN
    assert b"aligned" in lib.jspsr_last_error()
    assert lib.jspsr_summary_workspace_bytes(0, 1, 64, 1) == 0 and lib.jspsr_summary_workspace_bytes(1, 1, 2 ** 32, 2 ** 19) == 0
    assert launches(PREPARE, SELECT) == before
    with pytest.raises(ValueError):                                       # an empty window is refused before any call
        S.scores_pooled(x.view(1, 8, 8), x.view(1, 8, 8), segments=[[(0, 0, 0, 0, 8)]])
    a_before = launches(ASSEMBLE)
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert lib.jspsr_scenes_assemble_f32(None, x.data_ptr(), None, x.data_ptr(), off.data_ptr(), 64, 1, 1, 8, 0, 0, 0, 0.0, 1.0, None) == EINVAL
    assert lib.jspsr_scenes_assemble_f32(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), off.data_ptr(), 64, 0, 1, 8, 0, 0, 0, 0.0, 1.0, None) == EINVAL
    assert launches(ASSEMBLE) == a_before and launches(PREPARE, SELECT) == before
