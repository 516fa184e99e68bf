"""K25 on the MI355X: jspsr_resample_forward through `resample.resample_rasters` / `resize`, the stores built with
`lr_resample=` and `evaluate(resize_input=)`, against the numpy restatement tests/resample_ref.py.

Bounds.  Against the restatement every comparison is bit for bit: the kernel rounds each operation once, in the
restatement's order.  Against float64 F.interpolate on the CPU: |out - ref| <= 2^-23 |ref| + 12 * 2^-24 * sum |w_ij| |v_ij - c|
(resample_ref.tolerance) -- the last rounding, and the roundings of the longest path before it (one subtraction, two weight
roundings, two products, six additions, one spare), each relative to a term of that sum, which is formed in float64 here.
The stores are compared bit for bit with the by-hand route (fill on the coarse grid, resample, margin), all of it numpy."""
import numpy as np
import pytest
import torch

from jspsr_amd import data as D
from jspsr_amd import evaluate as EV
from jspsr_amd import infer as I
from jspsr_amd import losses as L
from jspsr_amd import resample as RS
from tests import batches_ref as B
from tests import resample_ref as R
from tests import voids_ref as V
from tests.test_infer_gpu import DEV, jspsr_model, launches, params
from tests.test_tiled_gpu import Pointwise, raster

pytestmark = pytest.mark.gpu

SHAPES = [((1, 1), (5, 3)), ((2, 3), (7, 5)), ((5, 4), (19, 15)), ((16, 16), (60, 60)), ((35, 19), (130, 70)),
          ((89, 89), (334, 334)), ((7, 7), (7, 7))]
MODES = ("bicubic", "bilinear")


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int32)


@pytest.fixture(scope="module")
def cases():
    """The rasters, their restatements and float64 references, computed once and left unchanged."""
    rng = np.random.default_rng(25)
    srcs = [R.terrain(rng, *s) for s, _ in SHAPES]
    want = {m: [R.resample(a, *d, m) for a, (_, d) in zip(srcs, SHAPES)] for m in MODES}
    ref64 = {m: [R.torch_ref(a, *d, m) for a, (_, d) in zip(srcs, SHAPES)] for m in MODES}
    return srcs, want, ref64


def one(a, dst, mode="bicubic", **kw):
    out = RS.resample_rasters(torch.from_numpy(a.reshape(-1)).to(DEV), [(0, *a.shape)], [dst], mode, **kw)
    return (out[0].view(*dst),) + tuple(out[1:])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES])
def test_one_raster_has_the_restatements_bits_and_is_torch_in_float64(cases, k, mode):
    srcs, want, ref64 = cases
    (src, dst), a = SHAPES[k], srcs[k]
    n0 = launches(b"resample")
    out, table = one(a, dst, mode)
    assert launches(b"resample") == n0 + 1 and table.tolist() == [[0, *dst]]
    got = out.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want[mode][k]))
    err = np.abs(got.astype(np.float64) - ref64[mode][k])
    tol = R.tolerance(ref64[mode][k], a, *dst, mode)
    print(f"{src} -> {dst} {mode}: max err {err.max():.3e}, max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol)
    if src == dst:
        assert np.array_equal(bits(got), bits(a))                                # the input's bits
    assert np.array_equal(bits(one(a, dst, mode)[0]), bits(got))                 # the same bits on a second run


@pytest.mark.parametrize("mode", MODES)
def test_mixed_shapes_in_one_call_have_the_same_bits_whatever_shares_the_call(cases, mode):
    srcs, want, _ = cases
    offs = np.concatenate([[0], np.cumsum([a.size for a in srcs])])
    assert any(o % 4 for o in offs[1:-1])                                        # flat offsets that are no multiple of 4
    flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in srcs])).to(DEV)
    table = [(int(offs[k]), *srcs[k].shape) for k in range(len(srcs))]
    n0 = launches(b"resample")
    dst, dst_table = RS.resample_rasters(flat, table, [d for _, d in SHAPES], mode)
    assert launches(b"resample") == n0 + 1                                       # ONE launch for the seven shapes
    assert any(int(o) % 4 for o in dst_table[1:, 0]) and dst.numel() == sum(h * w for _, (h, w) in SHAPES)
    got = dst.cpu().numpy()
    for k, (o, h, w) in enumerate(dst_table.tolist()):
        assert (h, w) == SHAPES[k][1] and np.array_equal(bits(got[o:o + h * w].reshape(h, w)), bits(want[mode][k])), k
    again, _ = RS.resample_rasters(flat, table, [d for _, d in SHAPES], mode)
    assert torch.equal(again.view(torch.int32), dst.view(torch.int32))
    order = [5, 0, 3, 6]                                                         # other neighbours, another order
    sub, sub_table = RS.resample_rasters(flat, [table[k] for k in order], [SHAPES[k][1] for k in order], mode)
    for pos, k in enumerate(order):
        o, h, w = sub_table[pos].tolist()
        assert np.array_equal(bits(sub[o:o + h * w].view(h, w)), bits(want[mode][k])), k


def test_resize_is_every_plane_resampled(cases):
    x = torch.from_numpy(np.stack([R.terrain(np.random.default_rng(s), 16, 9) for s in range(6)]).reshape(2, 3, 16, 9)).to(DEV)
    for mode in MODES:
        n0 = launches(b"resample")
        y = RS.resize(x, (60, 34), mode)
        assert launches(b"resample") == n0 + 1 and y.shape == (2, 3, 60, 34) and y.dtype == torch.float32
        for b in range(2):
            for c in range(3):
                assert np.array_equal(bits(y[b, c]), bits(R.resample(x[b, c].cpu().numpy(), 60, 34, mode))), (mode, b, c)
    for bad in ((15, 34), (60, 8)):
        with pytest.raises(ValueError, match="downsampling"):
            RS.resize(x, bad)


def test_clamp_holds_the_overshoot_of_a_step_edge():
    a = np.zeros((9, 12), np.float32)
    a[:, 6:] = 1000
    a[4:, :] = 1000 - a[4:, :]
    free = one(a, (33, 45))[0].cpu().numpy()
    held = one(a, (33, 45), clamp=[(0, 1000)])[0].cpu().numpy()
    assert free.min() < 0 and free.max() > 1000                                  # bicubic overshoots
    assert held.min() == 0 and held.max() == 1000
    assert np.array_equal(bits(free), bits(R.resample(a, 33, 45))) and np.array_equal(bits(held), bits(R.resample(a, 33, 45, clamp=(0, 1000))))
    dev = one(a, (33, 45), clamp=torch.tensor([[0.0, 1000.0]], device=DEV))[0].cpu().numpy()      # the clamp as a device tensor
    assert np.array_equal(bits(dev), bits(held))
    assert free.min() < -10 and free.max() > 1010
    lin = one(a, (33, 45), "bilinear")[0].cpu().numpy()
    assert lin.min() >= -1e-3 and lin.max() <= 1000 + 1e-3                       # bilinear does not, beyond an ulp of 1000 or two


@pytest.mark.parametrize("mode", MODES)
def test_void_plane_follows_the_centre_tap_and_a_nan_stays_within_two_source_pixels(mode):
    rng = np.random.default_rng(4)
    a = R.terrain(rng, 35, 19)
    v = (rng.random((35, 19)) < 0.05).astype(np.uint8)
    v[10:14, 3:6] = 1
    v[20, 9] = 1
    a[20, 9] = np.nan                                                            # a void the fill did not see
    n0 = launches(b"resample (void)")
    out, _, dv = one(a, (130, 70), mode, void=torch.from_numpy(v.reshape(-1)).to(DEV))
    assert launches(b"resample (void)") == n0 + 1
    assert dv.dtype == torch.uint8 and np.array_equal(dv.view(130, 70).cpu().numpy(), R.void_plane(v, 130, 70, mode))
    got = out.cpu().numpy()
    assert np.array_equal(got, R.resample(a, 130, 70, mode), equal_nan=True)
    assert np.array_equal(bits(np.nan_to_num(got)), bits(np.nan_to_num(one(a, (130, 70), mode)[0].cpu().numpy())))   # the plane changes no value
    ct = R.CENTRE[mode]
    iy = np.clip(R.axis_taps(35, 130, mode)[0].astype(int) + ct, 0, 34)
    ix = np.clip(R.axis_taps(19, 70, mode)[0].astype(int) + ct, 0, 18)
    far = np.maximum(np.abs(iy - 20)[:, None], np.abs(ix - 9)[None, :]) > 2
    assert np.isnan(got).any() and not np.isnan(got[far]).any()


# ---- the stores ------------------------------------------------------------------------------------------------------------
FINE3 = [(48, 80), (48, 80), (40, 40)]
COARSE3 = [(13, 22), (14, 21), (11, 11)]
NODATA = -32767.0
KINDS3 = ("image", "mask")


def coarse_scenes(voids: bool):
    fine = B.make_scenes(FINE3, seed=17)
    coarse = [s["lr_dem"].copy() for s in B.make_scenes(COARSE3, seed=18)]
    if voids:
        rs = np.random.RandomState(71)
        for j, a in enumerate(coarse):
            h, w = a.shape[:2]
            v = rs.rand(h, w) < 0.04
            if j == 0:
                v[:6, :7] = True                                                 # a corner deeper than fill_limit = 2
            kind = rs.randint(0, 3, (h, w))
            a[..., 0][v] = np.where(kind == 0, NODATA, np.where(kind == 1, np.nan, np.inf))[v]
    return fine, coarse


def build(fine, coarse, cls=I.InferenceScenes, **kw):
    p = {k: v for k, v in params(**kw).items() if k != "label_range" or cls is D.DeviceScenes}
    lists = {k: [s[k] for s in fine] for k in KINDS3 + (("hr_dem",) if cls is D.DeviceScenes else ())}
    return cls(lr_dem=coarse, coord=None, device=DEV, **lists, **p)


def by_hand(coarse, mode, relative, margin, limit):
    """The host route: fill on the coarse grid, resample with the clamp of the valid coarse range, margin on the fine grid."""
    filled, bases, voids, _ = V.by_hand_store(coarse, NODATA, relative, 0, limit)
    fine, fvoid, fout = [], [], []
    for a, f, v, (H, W) in zip(coarse, filled, voids, FINE3):
        good = a[..., 0][~v]
        fine.append(R.resample(f[..., 0], H, W, mode, clamp=(good.min(), good.max())))
        fvoid.append(R.void_plane(v, H, W, mode))
        fout.append(V.margin_ref(fvoid[-1], margin))
    return fine, bases, voids, fvoid, fout


@pytest.mark.parametrize("mode,relative,margin,limit", [("bicubic", True, 0, None), ("bicubic", True, 3, 2), ("bilinear", False, 3, None)])
def test_inference_store_is_the_by_hand_route(mode, relative, margin, limit):
    fine, coarse = coarse_scenes(True)
    want, bases, voids, fvoid, fout = by_hand(coarse, mode, relative, margin, limit)
    n0, f0 = launches(b"resample (void)"), launches(b"scene_fill_voids")
    S = build(fine, coarse, relative=relative, nodata=NODATA, void_margin=margin, fill_limit=limit, lr_resample=mode)
    assert launches(b"resample (void)") == n0 + 1 and launches(b"scene_fill_voids") == f0 + 1
    assert [tuple(s) for s in S.shapes] == FINE3 and [tuple(s) for s in S.lr_shapes] == COARSE3
    assert S.scene_table.cpu().tolist() == [[0, 48, 80], [3840, 48, 80], [7680, 40, 40]]
    assert [float(np.float32(b)) for b in S.base] == [float(np.float32(b)) for b in bases]
    assert S.void_counts == [int(v.sum()) for v in voids] and min(S.void_counts) > 0
    assert np.array_equal(bits(S.store["lr_dem"]), bits(np.concatenate([f.reshape(-1) for f in want])))
    assert bool(torch.isfinite(S.store["lr_dem"]).all())
    assert (S.void_out is S.void) == (margin == 0)
    for i in range(3):
        assert np.array_equal(S.void_mask(i).cpu().numpy(), fvoid[i] != 0), i
        assert np.array_equal(S.void_mask(i, out=True).cpu().numpy(), fout[i]), i
        lo, hi = S.lr_clamp[i]
        z = S.store["lr_dem"][S.scene_table[i, 0]:][:FINE3[i][0] * FINE3[i][1]]
        assert float(z.min()) >= lo >= np.float32(S.base[i]) and float(z.max()) <= hi
    if limit == 2 and relative:                                                  # the corner's far pixels hold the base
        assert float(S.store["lr_dem"][0]) == float(np.float32(bases[0]))


@pytest.fixture(scope="module")
def pair():
    """A store built with lr_resample and nodata, and the store a user builds from the downloaded resampled rasters."""
    fine, coarse = coarse_scenes(True)
    S = build(fine, coarse, nodata=NODATA, void_margin=2, lr_resample="bicubic")
    flat = S.store["lr_dem"].cpu().numpy()
    rasters = [flat[o:o + h * w].reshape(h, w, 1).copy() for (o, h, w) in S.scene_table.cpu().tolist()]
    H = build(fine, rasters, base=S.base)
    return S, H


def test_predictions_have_the_bits_of_a_store_of_host_resampled_scenes(pair):
    S, H = pair
    assert all(torch.equal(S.store[k], H.store[k]) for k in H.store) and S.base == H.base and S.shapes == H.shapes
    model, _ = jspsr_model()
    for m, kw in ((Pointwise(), dict(batch_size=2)), (Pointwise(), dict(batch_size=4, tile=32, overlap=8, trim=2)),
                  (Pointwise(), dict(batch_size=8, tta="d4")), (model, dict(batch_size=2))):
        want = I.predict_scenes(m, H, **kw)
        got = I.predict_scenes(m, S, mask_voids=False, **kw)
        assert got.offsets == want.offsets and got.shapes == want.shapes == FINE3
        assert torch.equal(got.buffer.view(torch.int32), want.buffer.view(torch.int32)), kw
    masked = I.predict_scenes(Pointwise(), S, batch_size=2)                       # mask_out reads the fine plane
    want = I.predict_scenes(Pointwise(), H, batch_size=2)
    for pos in range(3):
        out = S.void_mask(pos, out=True).cpu().numpy()
        assert out.any() and np.array_equal(raster(masked, pos).cpu().numpy(), np.where(out, np.float32(NODATA), raster(want, pos).cpu().numpy()))


def test_a_store_of_lr_dem_alone_takes_lr_shape():
    _, coarse = coarse_scenes(False)
    p = {k: v for k, v in params().items() if k != "label_range"}
    S = I.InferenceScenes(lr_dem=coarse[:2], device=DEV, lr_resample="bicubic", lr_shape=(48, 80), **p)
    assert S.void is None and S.shapes == [(48, 80), (48, 80)] and S.lr_shapes == COARSE3[:2]
    for i, a in enumerate(coarse[:2]):
        want = R.resample(a[..., 0], 48, 80, clamp=(a.min(), a.max()))
        assert np.array_equal(bits(S.store["lr_dem"][i * 3840:(i + 1) * 3840].view(48, 80)), bits(want)), i
    T = I.InferenceScenes(lr_dem=coarse, device=DEV, lr_resample="bilinear", lr_shape=FINE3, **p)
    assert [tuple(s) for s in T.shapes] == FINE3
    a = coarse[2][..., 0]
    assert np.array_equal(bits(T.store["lr_dem"][7680:].view(40, 40)), bits(R.resample(a, 40, 40, "bilinear", clamp=(a.min(), a.max()))))


def test_device_scenes_and_one_random_crop_batch():
    fine, coarse = coarse_scenes(False)
    S = build(fine, coarse, cls=D.DeviceScenes, lr_resample="bicubic")
    assert [tuple(s) for s in S.shapes] == FINE3 and [tuple(s) for s in S.lr_shapes] == COARSE3
    assert S.base == [np.min(a) for a in coarse]                                 # the base reads the coarse raster
    want = [R.resample(a[..., 0], H, W, clamp=(a.min(), a.max())) for a, (H, W) in zip(coarse, FINE3)]
    assert np.array_equal(bits(S.store["lr_dem"]), bits(np.concatenate([f.reshape(-1) for f in want])))
    Hd = build(fine, [f[..., None] for f in want], cls=D.DeviceScenes)           # host-resampled rasters passed as lr_dem
    Hd.base = list(S.base)
    batches = [next(iter(D.RandomCropBatches(st, 4, 32, rng=np.random.RandomState(5), sampler=[0, 1, 2, 1]))) for st in (S, Hd)]
    assert sorted(batches[0]) == sorted(batches[1])
    for k in ("lr_dem", "hr_dem", "image", "mask", "base"):
        assert torch.equal(batches[0][k].view(torch.int32), batches[1][k].view(torch.int32)), k
    assert batches[0]["meta"] == batches[1]["meta"] and batches[0]["lr_dem"].shape == (4, 1, 32, 32)


def test_without_the_keyword_mismatched_shapes_still_raise():
    fine, coarse = coarse_scenes(False)
    with pytest.raises(ValueError, match="does not match lr_dem"):
        build(fine, coarse)
    with pytest.raises(ValueError, match="does not match lr_dem"):
        build(fine, coarse, cls=D.DeviceScenes)


def test_evaluate_resizes_a_smaller_input():
    from tests.test_eval_gpu import IC, new_meter
    g = torch.Generator().manual_seed(9)
    lr = (torch.rand(2, 1, 32, 32, generator=g) * 0.5 + 0.2).to(DEV)
    gt = (torch.rand(2, 1, 64, 64, generator=g) * 0.5 + 0.2).to(DEV)
    batch = {"lr_dem": lr, "image": torch.zeros(2, 3, 64, 64, device=DEV), "mask": torch.zeros(2, 15, 64, 64, device=DEV),
             "hr_dem": gt, "base": None, "meta": [{}, {}]}

    class Fixed(torch.nn.Module):
        def forward(self, lr, image, mask):
            return torch.zeros(lr.shape[0], 1, 64, 64, device=lr.device) + 0.5

    with pytest.raises(NotImplementedError):
        EV.evaluate(Fixed(), [batch], L.get_criterion({"L1": 1}), new_meter(), "JSPSR", IC, compare_input=True)
    r = EV.evaluate(Fixed(), [batch], L.get_criterion({"L1": 1}), new_meter(), "JSPSR", IC, compare_input=True, resize_input="bicubic")
    direct = new_meter()
    direct.update(RS.resize(lr, (64, 64)), gt, meta=[{}, {}])
    assert len(r) == 4 and r[3] == direct.get_score() and r[3]["RMSE"] > 0
    ref = torch.nn.functional.interpolate(lr.cpu().double(), size=(64, 64), mode="bicubic", align_corners=False)
    assert float((RS.resize(lr, (64, 64)).cpu().double() - ref).abs().max()) <= 2 ** -22      # values below 1: a few ulp of 2^-24
