"""K20 on the MI355X: `metrics.batch_scores(valid=)` (jspsr_scores_batch_valid_forward) against the fp64 restatement
(tests/masked_eval_ref.py), torch's own order statistics on the boolean-indexed exact differences, and the unmasked call
(all-ones plane: the same bytes; rectangular plane: the contiguous cropped tile); garbage at the masked places, row
independence, repeatability, chaining, launch census, error codes; and `evaluate` / `fit` on a store whose ground truth has
voids (K19) with `PerformanceMeter(masked=True)`.

Inputs as tests/test_eval_gpu.py: exact_tiles -- linear scaling (0, 2) makes dh = 2 (pred - gt) exact, with ties, zeros and
negatives.  Tolerances of the sum columns are the unmasked tests' for the same columns: 1e-3 absolute for the two PSNR,
2e-3 + 1e-5 |ref| otherwise.  Where such a bound fails masked, the message says whether the unmasked call on the same tile
meets it."""
import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import evaluate as EV
from jspsr_amd import losses as L
from jspsr_amd import metrics as M
from jspsr_amd import optim as O
from jspsr_amd import train as TR
from jspsr_amd.ddp import GradReducer
from oracle import jspsr_ref as JR
from tests import batches_ref as BR
from tests import eval_ref as E
from tests import masked_eval_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LDS, STREAM = b"scores_batch (lds)", b"scores_batch (stream)"
V_LDS, V_STREAM = b"scores_batch_valid (lds)", b"scores_batch_valid (stream)"
STREAM_LAUNCHES = 27                                     # prepare, slope, reduce, 3 x 4 x (hist, scan)
LDS_SHAPES = [(37, 53, 0.0), (37, 53, 0.05), (128, 128, 0.0)]
STREAM_SHAPES = [(160, 150, 0.0), (150, 170, 0.05)]
SHAPES = [(s, V_LDS) for s in LDS_SHAPES] + [(s, V_STREAM) for s in STREAM_SHAPES]
SHAPE_IDS = [f"{h}x{w}b{int(b * 100)}" for (h, w, b), _ in SHAPES]
GARBAGE = (float("nan"), float("inf"), -float("inf"), -32767.0, 1e30)
MT = 256                                                 # the streaming kernels' workgroup: element i belongs to block (i // MT) % blocks


def launches(name):
    return _lib.load().jspsr_launch_count(name)


def exact_tiles(B, H, W, seed):
    """Tiles whose differences are exact under linear scaling (0, 2): dh = 2 (pred - gt).  Ties, zeros, negatives."""
    g_ = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, 1, H, W, generator=g_) * 0.5
    d = torch.randn(B, 1, H, W, generator=g_) * 0.01
    d[:, 0, :3] = 0.0
    d[:, 0, 5, ::2] = 0.0078125
    d[:, 0, 6, ::3] = -0.0078125
    pred = (gt + d).clamp(0, 1)
    return pred, gt


_TILES = {}


def tiles(B, H, W):
    """The CPU pair of a shape, made once and never changed."""
    if (B, H, W) not in _TILES:
        _TILES[B, H, W] = exact_tiles(B, H, W, seed=300 + B)
    return _TILES[B, H, W]


def crop(H, W, border):
    bh, bw = int(H * border), int(W * border)
    return bh, bw, H - 2 * bh, W - 2 * bw


def stream_blocks(n):
    return min(1024, max(1, -(-n // (MT * 8))))


def make_mask(kind, B, H, W, border, seed=0):
    """(B,1,H,W) uint8 CPU plane."""
    rs = np.random.RandomState(1000 + seed)
    bh, bw, h, w = crop(H, W, border)
    v = np.ones((B, 1, H, W), np.uint8)
    if kind.startswith("speckle"):
        v = (rs.rand(B, 1, H, W) >= int(kind[7:]) / 100.0).astype(np.uint8)
    elif kind == "half":
        v[..., W // 2:] = 0
        v[0, 0, : H // 2] = 1                                    # tile 0: an L shape, the others a half plane
    elif kind in ("n1", "n2", "n3"):
        v[:] = 0
        for b in range(B):
            for k in range(int(kind[1])):
                v[b, 0, bh + (5 + 7 * k + b) % h, bw + (3 + 11 * k + 2 * b) % w] = 1
    elif kind == "checker":
        v[:] = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint8)
    elif kind == "voidmid":
        v = (rs.rand(B, 1, H, W) >= 0.1).astype(np.uint8)
        v[B // 2] = 0
    elif kind in ("block1void", "lastblock"):
        n = h * w
        i = np.arange(n)
        blocks = stream_blocks(n)
        assert n > 20272 and blocks > 2 and n % MT != 0          # a streaming shape with a partial last block
        keep = ((i // MT) % blocks != 1) if kind == "block1void" else (i >= (n // MT) * MT)
        v[:] = 0
        v[:, 0, bh:bh + h, bw:bw + w] = keep.reshape(h, w).astype(np.uint8)
    else:
        assert kind == "ones"
    return torch.from_numpy(v)


def poison(t, valid, shift=0):
    out = t.clone()
    idx = torch.nonzero(valid.reshape(-1) == 0).reshape(-1)
    out.view(-1)[idx] = torch.tensor(GARBAGE, dtype=torch.float32)[(torch.arange(idx.numel()) + shift) % len(GARBAGE)]
    return out


def run(pred, gt, valid, border):
    s, c = M.batch_scores(pred.to(DEV), gt.to(DEV), 0.0, 2.0, border, False, valid=valid.to(DEV))
    assert s.shape == (pred.shape[0], 8) and s.dtype == torch.float32 and c.shape == (pred.shape[0], 3) and c.dtype == torch.int32
    return s.cpu(), c.cpu()


def sum_bound(col, ref):
    """The unmasked tests' bound of a sum column: 1e-3 absolute for the two PSNR, 2e-3 + 1e-5 |ref| otherwise."""
    return np.full(np.shape(ref), 1e-3) if col < 2 else 2e-3 + 1e-5 * np.abs(np.nan_to_num(ref))


def check(pred, gt, valid, border, label):
    """One masked call against the restatement (counts, sum columns) and torch's order statistics (bit-equal)."""
    B, _, H, W = pred.shape
    bh, bw, h, w = crop(H, W, border)
    got, cnt = run(poison(pred, valid), poison(gt, valid, 2), valid, border)
    want, wc = R.batch_scores(pred.numpy(), gt.numpy(), valid.numpy(), 0.0, 2.0, border, False)
    assert np.array_equal(cnt.numpy(), wc), (label, cnt, wc)
    g64 = got.numpy().astype(np.float64)
    assert np.array_equal(np.isnan(g64), np.isnan(want)), (label, g64, want)
    dh = (pred * 2.0 - gt * 2.0)[:, 0, bh:H - bh, bw:W - bw]
    vc = valid[:, 0, bh:H - bh, bw:W - bw] != 0
    for b in range(B):
        if wc[b, 0]:
            d = dh[b][vc[b]]
            med = torch.median(d)
            assert got[b, 3].item() == med.item(), (label, b)
            assert got[b, 4].item() == (1.4826 * torch.median((d - med).abs())).item(), (label, b)
            assert got[b, 5].item() == torch.kthvalue(d.abs(), 1 + round(0.95 * (d.numel() - 1))).values.item(), (label, b)
    for col in (0, 1, 2, 6, 7):
        ok = ~np.isnan(want[:, col])
        err = np.abs(g64[:, col] - want[:, col])
        tol = sum_bound(col, want[:, col])
        print(label, M.SCORE_COLUMNS[col], "max err", err[ok].max() if ok.any() else None)
        if not np.all((err <= tol)[ok]):                      # the same bound on the unmasked call for the same tiles: which of the two?
            plain = M.batch_scores(pred.to(DEV), gt.to(DEV), 0.0, 2.0, border, False).cpu().numpy().astype(np.float64)
            pw = E.batch_scores(pred.numpy(), gt.numpy(), 0.0, 2.0, border, False)
            perr = np.abs(plain[:, col] - pw[:, col])
            verdict = "meets" if np.all(perr <= sum_bound(col, pw[:, col])) else "also misses"
            raise AssertionError(f"{label} column {M.SCORE_COLUMNS[col]}: masked err {err} > {tol}; the unmasked call on the same "
                                 f"tiles {verdict} its bound (err {perr})")
    return got, cnt


# ---- masks x shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,label", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("kind", ["speckle1", "speckle50", "speckle99", "half", "n1", "n2", "n3"])
def test_masks_against_restatement_and_torch_order_statistics(shape, label, B, kind):
    H, W, border = shape
    pred, gt = tiles(B, H, W)
    valid = make_mask(kind, B, H, W, border, seed=B)
    if kind == "speckle50" and (H, W) == (37, 53):
        assert (R.batch_scores(pred.numpy(), gt.numpy(), valid.numpy(), 0.0, 2.0, border, False)[1][:, 1] > 0).all()     # precondition
    before = launches(label)
    got, cnt = check(pred, gt, valid, border, f"{kind} {shape} B={B}")
    assert launches(label) == before + (1 if label == V_LDS else STREAM_LAUNCHES)
    if kind[0] == "n":
        assert cnt[:, 0].tolist() == [int(kind[1])] * B and (cnt[:, 1:] == 0).all() and torch.isnan(got[:, 6:]).all()
        assert torch.isfinite(got[:, :6]).all()


@pytest.mark.parametrize("shape,label", SHAPES, ids=SHAPE_IDS)
def test_checkerboard_has_no_slope(shape, label):
    H, W, border = shape
    pred, gt = tiles(5, H, W)
    got, cnt = check(pred, gt, make_mask("checker", 5, H, W, border), border, f"checker {shape}")
    assert (cnt[:, 0] > 0).all() and (cnt[:, 1:] == 0).all()
    assert torch.isnan(got[:, 6:]).all() and torch.isfinite(got[:, :6]).all()


@pytest.mark.parametrize("shape,label", SHAPES, ids=SHAPE_IDS)
def test_void_tile_in_the_middle_of_a_batch(shape, label):
    H, W, border = shape
    pred, gt = tiles(5, H, W)
    valid = make_mask("voidmid", 5, H, W, border)
    got, cnt = check(pred, gt, valid, border, f"voidmid {shape}")
    assert torch.isnan(got[2]).all() and cnt[2].tolist() == [0, 0, 0]
    assert torch.isfinite(got[[0, 1, 3, 4]]).all() and (cnt[[0, 1, 3, 4]] > 0).all()
    # the neighbours are what they are without the void tile in the batch
    keep = [0, 1, 3, 4]
    rest, rc = run(poison(pred, valid)[keep], poison(gt, valid, 2)[keep], valid[keep], border)
    assert rest.numpy().tobytes() == got[keep].numpy().tobytes() and torch.equal(rc, cnt[keep])


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=SHAPE_IDS[len(LDS_SHAPES):])
@pytest.mark.parametrize("kind", ["block1void", "lastblock"])
def test_streaming_block_masks(shape, kind):
    H, W, border = shape
    pred, gt = tiles(5, H, W)
    _, _, h, w = crop(H, W, border)
    got, cnt = check(pred, gt, make_mask(kind, 5, H, W, border), border, f"{kind} {shape}")
    n = h * w
    voided = sum(1 for c in range(n // MT) if c % stream_blocks(n) == 1) * MT       # whole chunks of block 1 (the partial one is not its)
    assert (n // MT) % stream_blocks(n) != 1 and voided >= 8 * MT
    assert cnt[:, 0].tolist() == [n - voided if kind == "block1void" else n % MT] * 5


# ---- garbage, all ones, rectangle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,label", SHAPES, ids=SHAPE_IDS)
def test_garbage_at_masked_places_has_no_influence(shape, label):
    H, W, border = shape
    pred, gt = tiles(5, H, W)
    valid = make_mask("speckle50", 5, H, W, border, seed=9)
    valid[4] = make_mask("half", 1, H, W, border)[0]
    clean = run(pred, gt, valid, border)
    a = run(poison(pred, valid), poison(gt, valid, 2), valid, border)
    b = run(poison(pred, valid, 3), poison(gt, valid, 1), valid, border)
    only_gt = run(pred, poison(gt, valid, 4), valid, border)
    for other in (a, b, only_gt):
        assert other[0].numpy().tobytes() == clean[0].numpy().tobytes() and torch.equal(other[1], clean[1])
    assert torch.isfinite(clean[0][:, :6]).all() and (clean[1][:, 0] > 0).all()
    assert torch.equal(torch.isnan(clean[0][:, 6:]), clean[1][:, 1:] == 0)          # a slope column is NaN exactly where its count is 0
    # a bool plane and any nonzero byte are the same plane
    for plane in (valid.bool(), valid * 255, valid * 2):
        again = run(pred, gt, plane, border)
        assert again[0].numpy().tobytes() == clean[0].numpy().tobytes() and torch.equal(again[1], clean[1])


@pytest.mark.parametrize("shape", [s for s, _ in SHAPES] + [(142, 142, 0.0)], ids=SHAPE_IDS + ["142x142b0"])
@pytest.mark.parametrize("B", [1, 5])
def test_all_ones_plane_gives_the_unmasked_bytes(shape, B):
    H, W, border = shape
    _, _, h, w = crop(H, W, border)
    pred, gt = (t.to(DEV) for t in tiles(B, H, W))
    label, plain_label = (V_LDS, LDS) if h * w <= 142 * 142 else (V_STREAM, STREAM)
    n0, p0 = launches(label), launches(plain_label)
    plain = M.batch_scores(pred, gt, 0.0, 2.0, border, False)
    assert launches(plain_label) > p0 and launches(label) == n0
    masked, cnt = M.batch_scores(pred, gt, 0.0, 2.0, border, False, valid=torch.ones_like(pred, dtype=torch.uint8))
    assert launches(label) - n0 == launches(plain_label) - p0                    # the same path, the same number of launches
    assert masked.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    assert cnt.cpu().tolist() == [[h * w, (h - 2) * (w - 2), h * w]] * B
    # and under log scaling, the fixture's range
    plain = M.batch_scores(pred, gt, E.VMIN, E.VMAX, border, True)
    masked, _ = M.batch_scores(pred, gt, E.VMIN, E.VMAX, border, True, valid=torch.ones_like(pred, dtype=torch.bool))
    assert masked.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("shape,rect", [((37, 53, 0.0), (4, 30, 6, 45)), ((37, 53, 0.05), (3, 20, 5, 25)), ((128, 128, 0.0), (10, 100, 1, 127)),
                                        ((160, 150, 0.0), (2, 158, 3, 149)), ((150, 170, 0.05), (20, 60, 30, 90))])
def test_rectangle_mask_equals_unmasked_call_on_the_cropped_tile(shape, rect):
    """Both are fp64 sums of the same terms in another order, rounded once: within 2 fp32 ulp; the selections bit-equal."""
    H, W, border = shape
    y0, y1, x0, x1 = rect
    pred, gt = tiles(5, H, W)
    valid = torch.zeros(5, 1, H, W, dtype=torch.uint8)
    valid[..., y0:y1, x0:x1] = 1
    got, cnt = run(poison(pred, valid), poison(gt, valid, 1), valid, border)
    sub = M.batch_scores(pred[..., y0:y1, x0:x1].contiguous().to(DEV), gt[..., y0:y1, x0:x1].contiguous().to(DEV), 0.0, 2.0, 0.0,
                         False).cpu()
    hh, ww = y1 - y0, x1 - x0
    assert cnt.tolist() == [[hh * ww, (hh - 2) * (ww - 2), (hh - 2) * (ww - 2)]] * 5
    assert got[:, 3:6].numpy().tobytes() == sub[:, 3:6].numpy().tobytes()
    u = ulps(got[:, [0, 1, 2, 6]].numpy(), sub[:, [0, 1, 2, 6]].numpy())
    print(shape, rect, "ulp", u.max(0))
    assert (u <= 2).all(), u


# ---- independence, repeatability, chaining, census ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,label", [SHAPES[1], SHAPES[2], SHAPES[4]], ids=[SHAPE_IDS[1], SHAPE_IDS[2], SHAPE_IDS[4]])
def test_rows_runs_chains_and_census(shape, label):
    H, W, border = shape
    plain_label = LDS if label == V_LDS else STREAM
    per_call = 1 if label == V_LDS else STREAM_LAUNCHES
    pred, gt = tiles(5, H, W)
    valid = make_mask("speckle50", 5, H, W, border, seed=4)
    valid[1] = 0
    valid[3] = make_mask("speckle1", 1, H, W, border)[0]
    p, g, v = poison(pred, valid).to(DEV), poison(gt, valid, 2).to(DEV), valid.to(DEV)
    other = V_STREAM if label == V_LDS else V_LDS
    census = {}
    for B in (1, 5):
        n0, o0, p0 = launches(label), launches(other), launches(LDS) + launches(STREAM)
        M.batch_scores(p[:B], g[:B], 0.0, 2.0, border, False, valid=v[:B])
        census[B] = launches(label) - n0
        assert launches(other) == o0 and launches(LDS) + launches(STREAM) == p0      # the unmasked labels do not move
    assert census == {1: per_call, 5: per_call}
    n0 = launches(plain_label)
    M.batch_scores(p, torch.where(v != 0, g, torch.zeros_like(g)), 0.0, 2.0, border, False)
    assert launches(plain_label) - n0 == per_call                                    # the unmasked census, unchanged
    full, fc = M.batch_scores(p, g, 0.0, 2.0, border, False, valid=v)
    again, ac = M.batch_scores(p, g, 0.0, 2.0, border, False, valid=v)
    assert full.cpu().numpy().tobytes() == again.cpu().numpy().tobytes() and torch.equal(fc, ac)      # two runs, the same bits
    ones = [M.batch_scores(p[b:b + 1], g[b:b + 1], 0.0, 2.0, border, False, valid=v[b:b + 1]) for b in range(5)]
    assert torch.cat([o[0] for o in ones]).cpu().numpy().tobytes() == full.cpu().numpy().tobytes()   # row b of 5 == the B = 1 call
    assert torch.equal(torch.cat([o[1] for o in ones]), fc)
    # a row does not depend on the other tiles' masks either
    v2 = v.clone()
    v2[[0, 2, 4]] = 1
    mixed, mc = M.batch_scores(p.nan_to_num(0.0, 0.0, 0.0), g.nan_to_num(0.0, 0.0, 0.0), 0.0, 2.0, border, False, valid=v2)
    assert mixed[[1, 3]].cpu().numpy().tobytes() == full[[1, 3]].cpu().numpy().tobytes() and torch.equal(mc[[1, 3]], fc[[1, 3]])
    # back to back without a synchronisation == with one after every call
    torch.cuda.synchronize()
    chain = [M.batch_scores(p[b:b + 2], g[b:b + 2], 0.0, 2.0, border, False, valid=v[b:b + 2]) for b in (0, 2, 3) for _ in range(3)]
    torch.cuda.synchronize()
    for i, (s, c) in enumerate(chain):
        b = (0, 2, 3)[i // 3]
        assert s.cpu().numpy().tobytes() == full[b:b + 2].cpu().numpy().tobytes() and torch.equal(c, fc[b:b + 2])


# ---- error paths ----------------------------------------------------------------------------------------------------------
def test_error_paths_return_codes_and_launch_nothing():
    lib = _lib.load()
    pred, gt = (t.to(DEV) for t in exact_tiles(2, 32, 32, seed=3))
    valid = torch.ones(2, 1, 32, 32, dtype=torch.uint8, device=DEV)
    out = torch.zeros(2, 8, device=DEV)
    cnt = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    labels = (V_LDS, V_STREAM, LDS, STREAM)
    n0 = sum(launches(x) for x in labels)

    def call(B=2, H=32, W=32, border=0.0, vmin=0.0, vmax=2.0, p=pred.data_ptr(), g=gt.data_ptr(), v=valid.data_ptr(), o=out.data_ptr(),
             c=cnt.data_ptr(), w=ws.data_ptr()):
        return lib.jspsr_scores_batch_valid_forward(p, g, v, B, H, W, border, vmin, vmax, 0, o, c, w, s)

    assert call(v=None) == -1 and b"validity plane" in lib.jspsr_last_error()
    assert call(c=None) == -1 and call(B=0) == -1 and call(B=-3) == -1
    assert call(border=0.5) == -1 and call(border=-0.1) == -1 and call(border=float("nan")) == -1
    assert call(vmax=1.0) == -1 and call(vmin=5.0, vmax=5.5) == -1
    assert call(H=0) == -1 and call(p=None) == -1 and call(g=None) == -1 and call(o=None) == -1 and call(w=None) == -1
    assert call(H=2, W=32) == -1 and call(H=32, W=2) == -1 and call(H=20, W=4, border=0.45) == -1
    assert call(w=ws.data_ptr() + 4) == -2 and call(p=pred.data_ptr() + 2) == -2 and call(c=cnt.data_ptr() + 2) == -2
    assert b"scores_batch_valid_forward" in lib.jspsr_last_error()
    assert sum(launches(x) for x in labels) == n0
    torch.cuda.synchronize()
    assert (out == 0).all() and (cnt == 0).all()
    for bad in (valid[:, 0], valid[:1], valid.float(), valid.int(), valid.cpu(), valid[..., :31], valid.cpu().numpy()):
        with pytest.raises(ValueError, match="valid"):
            M.batch_scores(pred, gt, 0.0, 2.0, 0.0, False, valid=bad)
    with pytest.raises(_lib.JspsrHipError):
        M.batch_scores(pred, gt, 0.0, 1.0, valid=valid)
    assert sum(launches(x) for x in labels) == n0
    assert call(v=valid.data_ptr() + 1, B=1) == 0                             # the plane needs no alignment; valid arguments run
    torch.cuda.synchronize()
    assert cnt[0].tolist() == [1024, 900, 1024]


# ---- end to end: evaluate and fit on a store with voids ---------------------------------------------------------------
IC = {"lr_dem": 1, "image": 3, "mask": 15}
E2E_SHAPES = [(100, 100), (96, 96)]               # square: the tile cover is laid out from the width
METRICS = {"PSNR": {"package": "piq"}, "RMSE": {"package": "local"}, "Median": {"package": "local"}, "NMAD": {"package": "local"},
           "LE95": {"package": "local"}, "Slope": {"package": "local"}}
COLS = (0, 2, 3, 4, 5, 6)
ELEV = (BR.PARAMS["elev_min"], BR.PARAMS["elev_max"], BR.PARAMS["elev_log"])
LOSS = {"L1": 1.0, "L2": 1.0, "Grad": 0.1}


@pytest.fixture(scope="module")
def scenes():
    raw = BR.make_scenes(E2E_SHAPES, seed=51)
    rs = np.random.RandomState(52)
    for i, s in enumerate(raw):
        hr = s["hr_dem"].copy()
        h, w = hr.shape[:2]
        hr[5:30, w - 20:] = -32767.0                       # a lake that touches the border
        hr[40 + i:52, 10:33] = np.nan                      # a cloud
        hr[rs.rand(h, w) < 0.05] = -32767.0                # sensor dropouts
        s["hr_dem"] = hr
    kinds = {k: [s[k] for s in raw] for k in ("lr_dem", "hr_dem", "image", "mask")}
    return D.DeviceScenes(**kinds, device=DEV, hr_nodata=-32767, **BR.PARAMS)


def build():
    from jspsr_amd.JSPSR import Model
    m = Model(dict(IC, COP30=1), num_feature=8)
    m.load_state_dict(JR.make_state_dict(JR.jspsr_param_shapes(IC, 8), seed=53))
    m = m.to(DEV).train()
    red = GradReducer(m.parameters())
    red.watch_streams(m.side_streams("cuda"))
    opt = O.FlatSGD(red, lr=1e-3, momentum=0.9, weight_decay=1e-6)
    return m, red, opt, O.ConstantLR(opt), L.get_criterion(LOSS)


def masked_meter():
    return EV.PerformanceMeter(METRICS, ELEV[0], ELEV[1], border=0.05, elev_log=ELEV[2], masked=True)


def averages(rows, counts):
    out = {}
    for name, col in zip(METRICS, COLS):
        keep = counts[:, M.COUNT_OF_COLUMN[col]] > 0
        out[name] = sum(float(x) for x in rows[keep, col]) / int(keep.sum())
    return out


def test_evaluate_with_a_masked_meter_equals_the_loop_over_tiles(scenes):
    m, _, _, _, crit = build()
    m.eval()
    runs = {}
    for bs in (3, 1):
        meter = masked_meter()
        res = EV.evaluate(m, D.TileCropBatches(scenes, bs, 64, 4), crit, meter, "JSPSR", IC, compare_input=True)
        runs[bs] = (res, meter.table()[0], meter.counts())
    rows, rows_in, counts = [], [], []
    with torch.no_grad():
        for batch in D.TileCropBatches(scenes, 1, 64, 4):
            inputs, gt, _, _ = D.batch_pair(batch, "JSPSR", IC)
            assert not torch.isfinite(gt).all() or int(batch["valid"].sum()) == gt.numel()
            for src, dst in ((m(*inputs), rows), (inputs[0][:, 0:1], rows_in)):
                s, c = M.batch_scores(src, gt, ELEV[0], ELEV[1], 0.05, ELEV[2], valid=batch["valid"])
                dst.append(s.cpu().numpy())
            counts.append(c.cpu().numpy())
    rows, rows_in, counts = np.concatenate(rows), np.concatenate(rows_in), np.concatenate(counts)
    assert len(rows) == 8 and 0 < counts[:, 0].min() and counts[:, 0].max() < 58 * 58 + 1 and (counts[:, 0] < 58 * 58).any()
    (res1, table1, counts1), (res3, table3, counts3) = runs[1], runs[3]
    assert np.array_equal(counts1, counts) and np.array_equal(counts3, counts)
    assert table1.tobytes() == rows[:, COLS].tobytes()                              # batch 1: the very calls of the loop
    want, want_in = averages(rows, counts), averages(rows_in, counts)
    assert res1[0] == want and res1[3] == want_in
    assert all(np.isfinite(v) for v in want.values()) and all(np.isfinite(v) for v in want_in.values())
    # batch 3 == batch 1: the order statistics of a tile do not depend on the batch it came in; the model's own outputs do
    # (to rounding), so the bound is the batch / tile comparison's of tests/test_eval_gpu.py
    for a, b in ((res3[0], res1[0]), (res3[3], res1[3])):
        for k in a:
            assert abs(a[k] - b[k]) <= (1e-3 if k == "PSNR" else 1e-4 * abs(b[k]) + 1e-6), (k, a[k], b[k])
    assert res3[3] == res1[3]                                                        # the input's scores run no model: equal
    assert abs(res3[1] - res1[1]) <= 1e-4 * abs(res1[1]) + 1e-6
    # an unmasked meter would have scored the voids
    with pytest.raises(NotImplementedError, match="masked=True"):
        EV.evaluate(m, D.TileCropBatches(scenes, 3, 64, 4), crit,
                    EV.PerformanceMeter(METRICS, ELEV[0], ELEV[1], border=0.05, elev_log=ELEV[2]), "JSPSR", IC)


def test_fit_on_a_store_with_voids(scenes):
    m, red, opt, sch, crit = build()
    train = list(D.RandomCropBatches(scenes, 2, 64, rng=np.random.RandomState(6), sampler=[0, 1, 1, 0]))
    val = list(D.TileCropBatches(scenes, 3, 64, 4))
    assert len(train) == 2 and all("valid" in b for b in train + val)
    meter = masked_meter()
    p = dict(epochs=2, model_name="JSPSR", input_data=IC, scheduler_kwargs={"warmup_epoch": 0}, val_interval=1, val_start_epoch=1,
             best_metric="RMSE", early_stop={"patience": 3, "monitor": "val_loss"}, monitor_value=None, resume=False)
    history = TR.fit(p, m, train, val, crit, opt, sch, red, meter)
    assert len(history) == 3 and [h["epoch"] for h in history] == [0, 1, 2]
    for h in history:
        if h["epoch"] == 0 or h["evaluated"]:
            assert list(h["scores"]) == list(METRICS) and all(np.isfinite(v) for v in h["scores"].values()), h
            assert np.isfinite(h["val_loss"])
    assert all(np.isfinite(v) for v in history[0]["input_scores"].values())
    assert history[1]["evaluated"] and history[2]["evaluated"] and np.isfinite(history[2]["train_loss"])
    # the counts of the last evaluation: the store's valid pixels under the cover, inside the meter's border crop
    bh = int(64 * 0.05)
    under = sum(int(b["valid"][..., bh:64 - bh, bh:64 - bh].sum()) for b in val)
    counts = meter.counts()
    assert counts.shape == (8, 3) and int(counts[:, 0].sum()) == under and 0 < under < 8 * 58 * 58
