"""K10 on the MI355X: `metrics.batch_scores` (jspsr_scores_batch_forward) against the reference-made fixture
(tests/golden/g12_eval.npz), the fp64 restatement (tests/eval_ref.py) and the one-tile path (`metrics.tile_scores`); its
launch census, determinism and error codes; and `evaluate.evaluate` over device-made validation batches.

Column 7 (the kornia slope) has no reference-made number (kornia is not installed where the fixture is made): it is held
to the restatement only."""
import os

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import evaluate as EV
from jspsr_amd import losses as L
from jspsr_amd import metrics as M
from tests import batches_ref as R
from tests import eval_ref as E
from tests import fixtures as Fx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g12_eval.npz")
DEV = "cuda:0"
CASES = [(name, border, lg) for name in E.SETS for border in E.BORDERS for lg in (True, False)]
REF_COLUMNS = {"PSNR_local": 1, "RMSE": 2, "Median": 3, "NMAD": 4, "LE95": 5, "Slope_local": 6}
LDS, STREAM = b"scores_batch (lds)", b"scores_batch (stream)"


def launches(name):
    return _lib.load().jspsr_launch_count(name)


@pytest.fixture(scope="module")
def g12():
    z = dict(np.load(GOLDEN))
    for name in E.SETS:       # fail, never skip, if the inputs do not regenerate
        assert E.checksum(E.tiles(name)) == float(z[f"{name}_checksum"]), name
    return z


def exact_tiles(B, H, W, seed):
    """Tiles whose differences are exact under linear scaling (0, 2): dh = 2 (pred - gt).  Ties, zeros, negatives."""
    g_ = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, 1, H, W, generator=g_) * 0.5
    d = torch.randn(B, 1, H, W, generator=g_) * 0.01
    d[:, 0, :3] = 0.0
    d[:, 0, 5, ::2] = 0.0078125
    d[:, 0, 6, ::3] = -0.0078125
    pred = (gt + d).clamp(0, 1)
    return pred.to(DEV), gt.to(DEV)


# ---- 4: against the fixture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,border,lg", CASES)
def test_batch_scores_match_reference_meters(g12, name, border, lg):
    key = E.case_key(name, border, lg)
    pred, gt = E.tiles(name)
    before = launches(LDS)
    got = M.batch_scores(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), E.VMIN, E.VMAX, border, lg)
    assert launches(LDS) == before + 1
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == (pred.shape[0], len(M.SCORE_COLUMNS)) and M.SCORE_COLUMNS == E.COLUMNS
    for metric, col in REF_COLUMNS.items():
        ref = g12[f"{key}_{metric}"]
        err = np.abs(got[:, col] - ref)
        print(key, metric, "max err", err.max())
        assert np.all(err <= 2e-3 + 1e-5 * np.abs(ref)), (key, metric, got[:, col], ref)
    want = E.batch_scores(pred, gt, E.VMIN, E.VMAX, border, lg)
    print(key, "vs restatement, max err per column", np.abs(got - want).max(0))
    assert np.all(np.abs(got[:, 7] - want[:, 7]) <= 2e-3 + 1e-5 * np.abs(want[:, 7])), (key, got[:, 7], want[:, 7])
    assert np.all(np.abs(got[:, 0] - want[:, 0]) <= 1e-3), (key, got[:, 0], want[:, 0])


# ---- 5: against the one-tile path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,border,path", [(37, 53, 0.0, LDS), (37, 53, 0.05, LDS), (128, 128, 0.05, LDS), (128, 128, 0.0, LDS),
                                               (512, 384, 0.05, STREAM), (160, 150, 0.0, STREAM)])
@pytest.mark.parametrize("B", [1, 5, 50])
def test_batch_scores_equal_tile_scores(H, W, border, path, B):
    pred, gt = exact_tiles(B, H, W, seed=100 + B)
    before = launches(path)
    got = M.batch_scores(pred, gt, 0.0, 2.0, border, False)
    assert launches(path) > before
    one = torch.stack([M.tile_scores(pred[b:b + 1], gt[b:b + 1], 0.0, 2.0, border, False) for b in range(B)])
    got, one = got.cpu(), one.cpu()
    assert torch.equal(got[:, 3:6], one[:, 2:5]), (got[:, 3:6] - one[:, 2:5]).abs().max()      # Median, NMAD, LE95: bit-equal
    assert (got[:, 0] - one[:, 0]).abs().max() < 1e-3
    assert ((got[:, 2] - one[:, 1]).abs() <= 1e-4 * one[:, 1].abs() + 1e-6).all()
    # and the torch formulas on the exact differences
    bh, bw = int(H * border), int(W * border)
    dh = (pred * 2.0 - gt * 2.0)[:, 0, bh:H - bh, bw:W - bw].reshape(B, -1)
    for b in (0, B - 1):
        med = torch.median(dh[b])
        assert got[b, 3].item() == med.item()
        assert got[b, 4].item() == (1.4826 * torch.median((dh[b] - med).abs())).item()
        assert got[b, 5].item() == torch.kthvalue(dh[b].abs(), 1 + round(0.95 * (dh.shape[1] - 1))).values.item()


def test_log_scaling_equals_tile_scores_bitwise():
    """The same de-scaling expressions as the one-tile kernel: under log scaling too the order statistics are the same bits."""
    pred, gt = (torch.from_numpy(a).to(DEV) for a in E.tiles("sq"))
    for border in (0.05, 0.0):
        got = M.batch_scores(pred, gt, E.VMIN, E.VMAX, border, True).cpu()
        one = torch.stack([M.tile_scores(pred[b:b + 1], gt[b:b + 1], E.VMIN, E.VMAX, border, True) for b in range(pred.shape[0])]).cpu()
        assert torch.equal(got[:, 3:6], one[:, 2:5])
        assert (got[:, 0] - one[:, 0]).abs().max() < 1e-3 and ((got[:, 2] - one[:, 1]).abs() <= 1e-4 * one[:, 1]).all()


def test_psnr_local_is_100_on_equal_tiles():
    gt = torch.rand(2, 1, 40, 40, device=DEV)
    got = M.batch_scores(gt.clone(), gt, E.VMIN, E.VMAX, 0.0, True).cpu()
    assert (got[:, 1] == 100.0).all() and (got[:, 2:] == 0).all() and (got[:, 0] - 80.0).abs().max() < 1e-3


# ---- 6: launch census, determinism ---------------------------------------------------------------------------------
def test_launch_census_and_row_independence():
    counts = {}
    for B in (1, 50):
        pred, gt = exact_tiles(B, 128, 128, seed=7)
        n0 = launches(LDS)
        s0 = launches(STREAM)
        M.batch_scores(pred, gt, E.VMIN, E.VMAX, 0.0, True)
        counts[B] = launches(LDS) - n0
        assert launches(STREAM) == s0
    assert counts == {1: 1, 50: 1}
    stream = {}
    for B in (1, 8):
        pred, gt = exact_tiles(B, 150, 170, seed=8)
        n0, l0 = launches(STREAM), launches(LDS)
        M.batch_scores(pred, gt, E.VMIN, E.VMAX, 0.05, True)
        stream[B] = launches(STREAM) - n0
        assert launches(LDS) == l0
    assert stream[1] == stream[8] > 0
    for shape, B in (((128, 128), 50), ((150, 170), 8)):
        pred, gt = exact_tiles(B, *shape, seed=9)
        pred[3, 0, 60, 60] = 1.4
        full = M.batch_scores(pred, gt, E.VMIN, E.VMAX, 0.05, True)
        again = M.batch_scores(pred, gt, E.VMIN, E.VMAX, 0.05, True)
        assert torch.equal(full, again)                                           # two runs, the same bits
        rows = torch.cat([M.batch_scores(pred[b:b + 1], gt[b:b + 1], E.VMIN, E.VMAX, 0.05, True) for b in range(B)])
        assert torch.equal(full, rows)                                            # row b of B == the B = 1 call on tile b
        # back to back without a synchronisation == with one after every call
        torch.cuda.synchronize()
        chain = [M.batch_scores(pred[b:b + 4], gt[b:b + 4], E.VMIN, E.VMAX, 0.05, True) for b in range(0, B, 4) for _ in range(3)]
        torch.cuda.synchronize()
        for i, c in enumerate(chain):
            b = (i // 3) * 4
            assert torch.equal(c, full[b:b + 4])


# ---- 7: error paths -------------------------------------------------------------------------------------------------
def test_error_paths_return_codes_and_launch_nothing():
    lib = _lib.load()
    pred, gt = exact_tiles(2, 32, 32, seed=3)
    out = torch.zeros(2, 8, device=DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    n0 = launches(LDS) + launches(STREAM)

    def call(B=2, H=32, W=32, border=0.0, vmin=0.0, vmax=2.0, p=pred.data_ptr(), g=gt.data_ptr(), o=out.data_ptr(), w=ws.data_ptr()):
        return lib.jspsr_scores_batch_forward(p, g, B, H, W, border, vmin, vmax, 0, o, w, s)

    assert call(B=0) == -1 and call(B=-3) == -1
    assert call(border=0.5) == -1 and call(border=-0.1) == -1 and call(border=float("nan")) == -1
    assert call(vmax=1.0) == -1 and call(vmin=5.0, vmax=5.5) == -1
    assert call(H=0) == -1 and call(p=None) == -1 and call(o=None) == -1 and call(w=None) == -1
    assert call(H=2, W=32) == -1 and call(H=32, W=2) == -1                   # fewer than 3 rows / columns
    assert call(H=20, W=4, border=0.45) == -1                                 # 2 x 2 left
    assert call(w=ws.data_ptr() + 4) == -2 and call(p=pred.data_ptr() + 2) == -2
    assert b"scores_batch_forward" in lib.jspsr_last_error()
    assert lib.jspsr_scores_batch_workspace_bytes(0, 32, 32) == 0 and lib.jspsr_scores_batch_workspace_bytes(2, 0, 32) == 0
    assert lib.jspsr_scores_batch_workspace_bytes(2, 128, 128) > 0
    assert lib.jspsr_scores_batch_workspace_bytes(2, 512, 512) >= 2 * 2 * 512 * 512 * 4
    assert launches(LDS) + launches(STREAM) == n0
    torch.cuda.synchronize()
    assert (out == 0).all()
    with pytest.raises(ValueError):
        M.batch_scores(pred[:, 0], gt[:, 0], 0.0, 2.0)
    with pytest.raises(ValueError):
        M.batch_scores(pred.cpu(), gt.cpu(), 0.0, 2.0)
    with pytest.raises(_lib.JspsrHipError):
        M.batch_scores(pred, gt, 0.0, 1.0)
    assert call() == 0                                                        # and the same arguments, valid, run
    torch.cuda.synchronize()


# ---- PerformanceMeter on the device --------------------------------------------------------------------------------
def test_performance_meter_gpu_matches_fixture_and_cpu(g12):
    cfg = {"PSNR": {"package": "local"}, "RMSE": {"package": "local"}, "Median": {}, "NMAD": {}, "LE95": {},
           "Slope": {"package": "local"}, "SSIM": {"package": "local"}}
    names = {"PSNR": "PSNR_local", "RMSE": "RMSE", "Median": "Median", "NMAD": "NMAD", "LE95": "LE95", "Slope": "Slope_local",
             "SSIM": "SSIM_local"}
    pred, gt = (torch.from_numpy(a).to(DEV) for a in E.tiles("sq"))
    key = E.case_key("sq", 0.05, True)
    tables = []
    for bs in (1, 3, 8):
        meter = EV.PerformanceMeter(cfg, E.VMIN, E.VMAX, border=0.05, elev_log=True)
        for lo in range(0, 8, bs):
            meter.update(pred[lo:lo + bs], gt[lo:lo + bs], meta=[{"id": i} for i in range(lo, min(lo + bs, 8))])
        for k, v in meter.get_score().items():
            ref = float(g12[f"{key}_avg_{names[k]}"])
            assert abs(v - ref) <= 2e-3 + 1e-5 * abs(ref), (bs, k, v, ref)
        assert [i for i, _ in meter.worst("RMSE")] == list(g12[f"{key}_worst_index"])
        tables.append(meter.table()[0])
    assert np.array_equal(tables[0][:, :6], tables[1][:, :6]) and np.array_equal(tables[0][:, :6], tables[2][:, :6])
    assert np.allclose(tables[0][:, 6], tables[2][:, 6], rtol=0, atol=1e-6)


# ---- 8: evaluate() ---------------------------------------------------------------------------------------------------
IC = Fx.MSK
METRICS = {"PSNR": {"package": "piq"}, "RMSE": {"package": "local"}, "Median": {"package": "local"},
           "NMAD": {"package": "local"}, "LE95": {"package": "local"}}
ELEV = dict(elev_min=R.PARAMS["elev_min"], elev_max=R.PARAMS["elev_max"], elev_log=R.PARAMS["elev_log"])


@pytest.fixture(scope="module")
def small_model():
    from jspsr_amd.JSPSR import Model
    z = Fx.load(os.path.join(HERE, "golden"), "g4_msk_nf8_b2_64_eval.npz")
    sd, _, _ = Fx.regen_jspsr(z, IC)
    m = Model(dict(IC, COP30=1), num_feature=int(z["nf"]))
    m.load_state_dict(Fx.as_f32(sd))
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def scenes():
    raw = R.make_scenes([(150, 150), (140, 140)], seed=23)
    kinds = {k: [s[k] for s in raw] for k in ("lr_dem", "hr_dem", "image", "mask")}
    return D.DeviceScenes(**kinds, device=DEV, ids=["s-0-a-b", "s-1-a-b"], **R.PARAMS)


def new_meter():
    return EV.PerformanceMeter(METRICS, ELEV["elev_min"], ELEV["elev_max"], border=0.05, elev_log=ELEV["elev_log"])


def close(a, b, what):
    """The bounds of the batch / tile comparison: 1e-3 absolute on PSNR, 1e-4 relative elsewhere."""
    for k in a:
        tol = 1e-3 if k == "PSNR" else 1e-4 * abs(b[k]) + 1e-6
        assert abs(a[k] - b[k]) <= tol, (what, k, a[k], b[k])


def test_evaluate_batch8_equals_batch1_and_the_meter_loop(small_model, scenes, monkeypatch):
    crit_cfg = {"L1": 1, "L2": 1, "Grad": 0.1}
    runs = {}
    for bs in (1, 8):
        batches = D.TileCropBatches(scenes, bs, 64, 9)                 # 18 tiles: the last batch of 8 holds 2
        runs[bs] = EV.evaluate(small_model, batches, L.get_criterion(crit_cfg), new_meter(), "JSPSR", IC)
    (s1, t1, c1), (s8, t8, c8) = runs[1], runs[8]
    assert list(s1) == list(METRICS) and list(c1) == list(crit_cfg)
    close(s8, s1, "scores 8 vs 1")
    close(dict(c8, Total=t8), dict(c1, Total=t1), "losses 8 vs 1")
    # per-sample predictions at batch 8 and batch 1
    p1 = torch.cat([small_model(*D.batch_pair(b, "JSPSR", IC)[0]) for b in D.TileCropBatches(scenes, 1, 64, 9)])
    p8 = torch.cat([small_model(*D.batch_pair(b, "JSPSR", IC)[0]) for b in D.TileCropBatches(scenes, 8, 64, 9)])
    for i in range(p1.shape[0]):
        assert Fx.rel(p8[i], p1[i]) < 1e-4, i
    # the loop the one-tile API allows: Meter + criterion + .item() per tile
    meter, crit = M.Meter(ELEV["elev_min"], ELEV["elev_max"], border=0.05, elev_log=ELEV["elev_log"]), L.get_criterion(crit_cfg)
    sums, n = {}, 0
    with torch.no_grad():
        for b in D.TileCropBatches(scenes, 1, 64, 9):
            crit.reset()
            inputs, gt, _, _ = D.batch_pair(b, "JSPSR", IC)
            pred = small_model(*inputs)
            for k, v in crit(pred, gt).items():
                sums[k] = sums.get(k, 0.0) + v.item()
            meter.update(pred, gt)
            n += 1
    assert n == 18
    close(s8, meter.scores(), "scores vs Meter")
    close(dict(c8, Total=t8), {k: v / n for k, v in sums.items()}, "losses vs the batch-1 loop")

    # one host synchronisation per pass, counted
    calls = {"n": 0}

    def counted(fn):
        def wrapper(*a, **k):
            calls["n"] += 1
            return fn(*a, **k)
        return wrapper

    batches = D.TileCropBatches(scenes, 8, 64, 9)
    crit, meter = L.get_criterion(crit_cfg), new_meter()
    list(batches)                                                    # the tile table is uploaded before the count starts
    monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "item", counted(torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "cpu", counted(torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "tolist", counted(torch.Tensor.tolist))
    s, t, c = EV.evaluate(small_model, batches, crit, meter, "JSPSR", IC, compare_input=False)
    meter.worst("RMSE")
    meter.table()
    monkeypatch.undo()
    assert calls["n"] == 1, calls
    close(s, s8, "counted pass")


def test_evaluate_berhu_and_compare_input(small_model, scenes):
    cfg = {"L1": 1.0, "Berhu": 0.5}
    r1 = EV.evaluate(small_model, D.TileCropBatches(scenes, 1, 64, 9), L.get_criterion(cfg), new_meter(), "JSPSR", IC)
    r8 = EV.evaluate(small_model, D.TileCropBatches(scenes, 8, 64, 9), L.get_criterion(cfg), new_meter(), "JSPSR", IC,
                     compare_input=True)
    assert len(r1) == 3 and len(r8) == 4 and list(r8[2]) == ["L1", "Berhu"]
    close(dict(r8[2], Total=r8[1]), dict(r1[2], Total=r1[1]), "BerHu at batch 8 vs batch 1")
    # BerHu over a whole batch is a different number (its threshold is the batch's maximum): the per-sample feed matters
    crit = L.get_criterion(cfg)
    with torch.no_grad():
        b = next(iter(D.TileCropBatches(scenes, 8, 64, 9)))
        inputs, gt, _, _ = D.batch_pair(b, "JSPSR", IC)
        pred = small_model(*inputs)
        whole = crit(pred, gt)["Berhu"].item()
        single = np.mean([L.get_criterion(cfg)(pred[i:i + 1], gt[i:i + 1])["Berhu"].item() for i in range(8)])
    assert abs(whole - single) > 1e-4 * abs(single)
    # the input's score == a meter fed with the LR DEM directly
    direct = new_meter()
    for b in D.TileCropBatches(scenes, 5, 64, 9):
        direct.update(b["lr_dem"], b["hr_dem"])
    close(r8[3], direct.get_score(), "input score")
    assert abs(r8[3]["RMSE"] - r8[0]["RMSE"]) > 0
    small = {"lr_dem": torch.zeros(1, 1, 32, 32, device=DEV), "image": torch.zeros(1, 3, 64, 64, device=DEV),
             "mask": torch.zeros(1, 15, 64, 64, device=DEV), "hr_dem": torch.zeros(1, 1, 64, 64, device=DEV), "base": None, "meta": [{}]}

    class Fixed(torch.nn.Module):
        def forward(self, lr, image, mask):
            return torch.zeros(lr.shape[0], 1, 64, 64, device=lr.device) + 0.5

    with pytest.raises(NotImplementedError):
        EV.evaluate(Fixed(), [small], L.get_criterion({"L1": 1}), new_meter(), "JSPSR", IC, compare_input=True)
