"""K13 on the MI355X: jspsr_scene_prepare / jspsr_scene_finish through jspsr_amd.infer, against the numpy restatement of
upscale_dem's steps (tests/infer_ref.py), K9 (`DeviceScenes.make`), `tiles.add_padding`, `metrics.descale_data` and the CPU
oracle's models.

Bounds.  Image, mask, canopy, coord and every finish output: compared with == (NaN positions equal).  The DEM: DEM_TOL of
tests/test_batches_gpu.py (device logf against numpy's fp32 log, one ulp divided by log(1013)).  Model outputs against the
fp64 oracle: tests/test_model_gpu.py's fp32 eval bound, max |pred - ref| < 1e-4 max |ref|."""
import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import infer as I
from jspsr_amd import metrics as M
from jspsr_amd import summary as S
from jspsr_amd import tiles as T
from oracle import jspsr_ref as O
from tests import batches_ref as B
from tests import infer_ref as R
from tests.test_batches_gpu import DEM_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# scene (H, W), pad, multiple -> frame
GEOMETRIES = [((40, 40), 12, 8, (64, 64)), ((37, 53), 5, 8, (48, 64)), ((37, 53), 0, 8, (40, 56)), ((9, 7), 6, 1, (21, 19))]
CONFIGS = [  # store parameters, concat
    (dict(), False),
    (dict(elev_log=False, relative=False, image_range="[-1, 1]", scale_mask=False), True),
    (dict(relative=False, image_range="[0, 255]"), False),
    (dict(elev_log=False), True),
]
KINDS = ("lr_dem", "image", "mask", "canopy", "coord")


def launches(name):
    return _lib.load().jspsr_launch_count(name)


def params(**kw):
    return dict(B.PARAMS, **kw)


def store(scenes, kinds=("lr_dem", "image", "mask", "canopy"), coord="local", hr=False, **kw):
    p = {k: v for k, v in params(**kw).items() if k != "label_range"}
    lists = {k: [s[k] for s in scenes] for k in kinds}
    if hr:
        return D.DeviceScenes(hr_dem=[s["hr_dem"] for s in scenes], coord=coord, device=DEV, label_range=None, **lists, **p)
    return I.InferenceScenes(coord=coord, device=DEV, **lists, **p)


def reference(scenes, p, n, multiple, kinds=KINDS):
    out = []
    for s in scenes:
        h, w = s["lr_dem"].shape[:2]
        full = dict({k: s[k] for k in kinds if k != "coord"}, **({"coord": B.local_coord(h, w)} if "coord" in kinds else {}))
        out.append(R.model_inputs(full, p, n, multiple))
    return out


def check_inputs(got: dict, refs: list, where):
    for kind, t in got.items():
        g = t.cpu().numpy()
        for b, ref in enumerate(refs):
            v = ref[kind]
            assert g[b].shape == v.shape, (where, kind, g[b].shape, v.shape)
            if kind == "lr_dem":
                err = np.abs(g[b].astype(np.float64) - v.astype(np.float64)).max()
                assert err <= DEM_TOL, (where, kind, b, err)
            else:
                assert np.array_equal(g[b], v), (where, kind, b, np.argwhere(g[b] != v)[:4])


def split(inputs, scenes_obj, concat):
    kinds = [k for k in KINDS if k in scenes_obj.channels]
    if not concat:
        return dict(zip(kinds, inputs))
    out, c0 = {}, 0
    for k in kinds:
        out[k] = inputs[0][:, c0:c0 + scenes_obj.channels[k]]
        c0 += scenes_obj.channels[k]
    assert c0 == inputs[0].shape[1]
    return out


# ---- prepare -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n,multiple,frame", GEOMETRIES)
def test_prepare_values(shape, n, multiple, frame):
    scenes = B.make_scenes([shape] * 3, seed=sum(shape) + n)
    for kw, concat in CONFIGS:
        Sc = store(scenes, **kw)
        assert len({float(b) for b in Sc.base}) == (3 if params(**kw)["relative"] else 1)
        n0 = launches(b"scene_prepare")
        inputs, fr = I.prepare(Sc, [2, 0, 1], n, multiple, concat=concat)
        assert launches(b"scene_prepare") == n0 + 1
        assert (fr.Hp, fr.Wp) == frame and (fr.top, fr.left, fr.H, fr.W) == (n, n) + shape
        assert len(inputs) == (1 if concat else 5) and all(t.dtype == torch.float32 and t.is_contiguous() for t in inputs)
        refs = reference([scenes[i] for i in (2, 0, 1)], params(**kw), n, multiple)
        check_inputs(split(inputs, Sc, concat), refs, (shape, n, kw))


@pytest.mark.parametrize("kw,concat", CONFIGS)
def test_prepare_shares_k9_bits_and_pads_as_add_padding(kw, concat):
    """The square scene, unpadded: K9's whole-scene crop, bit for bit, for every kind -- the shared arithmetic.  Padded by 12:
    `tiles.add_padding` of the unpadded result."""
    scenes = B.make_scenes([(40, 40)] * 3, seed=77)
    Sc = store(scenes, hr=True, **kw)
    plain, fr = I.prepare(Sc, [1, 2, 0], 0, 1, concat=False)
    assert (fr.Hp, fr.Wp, fr.top, fr.left) == (40, 40, 0, 0)
    got = split(plain, Sc, False)
    table = torch.tensor([[s, 0, 0, 0, np.float32(Sc.base[s]).view(np.int32), 0, 0, 0] for s in (1, 2, 0)], dtype=torch.int32, device=DEV)
    outs = {k: (torch.full((3, Sc.channels[k], 40, 40), -7.0, device=DEV), 0) for k in Sc.kinds}
    Sc.make(table, 40, outs)
    for k in KINDS:
        assert torch.equal(got[k], outs[k][0]), (kw, k)
    padded, fr = I.prepare(Sc, [1, 2, 0], 12, 1, concat=concat)
    assert (fr.Hp, fr.Wp, fr.top, fr.left) == (64, 64, 12, 12)
    for k, t in split(padded, Sc, concat).items():
        for b in range(3):
            assert torch.equal(t[b], T.add_padding(got[k][b], 12)), (kw, k, b)


@pytest.mark.parametrize("guard", [5, 8])
@pytest.mark.parametrize("shape,n,multiple,frame", GEOMETRIES)
def test_prepare_writes_nothing_outside_its_channels(shape, n, multiple, frame, guard):
    """The outputs are channel slices of one larger tensor filled with a sentinel, one spare channel on either side of each
    sample, starting `guard` elements into the allocation (5: no 16-byte alignment; 8: aligned)."""
    scenes = B.make_scenes([shape] * 3, seed=5)
    Sc = store(scenes)
    want, fr = I.prepare(Sc, [0, 1, 2], n, multiple, concat=True)
    C, (Hp, Wp) = want[0].shape[1], frame
    numel = 3 * (C + 2) * Hp * Wp
    big = torch.full((numel + 2 * guard,), -7.0, device=DEV)
    view = big[guard:guard + numel].view(3, C + 2, Hp, Wp)
    assert view.data_ptr() == big.data_ptr() + 4 * guard
    outs, c0 = {}, 1
    for k in KINDS:
        outs[k] = (view, c0)
        c0 += Sc.channels[k]
    rows, cols, _ = I._device_maps(shape[0], shape[1], n, multiple, Sc.device)
    table = torch.tensor([[s, np.float32(Sc.base[s]).view(np.int32)] for s in range(3)], dtype=torch.int32, device=DEV)
    I.launch_prepare(Sc, table, rows, cols, Hp, Wp, outs)
    assert torch.equal(view[:, 1:C + 1], want[0])
    assert bool((view[:, 0] == -7.0).all()) and bool((view[:, C + 1] == -7.0).all())
    assert bool((big[:guard] == -7.0).all()) and bool((big[guard + numel:] == -7.0).all())


# ---- finish ------------------------------------------------------------------------------------------------------------
def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal values, NaN at the same places."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0),
                                                                                             torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("elev_log", [True, False])
@pytest.mark.parametrize("shape,n,multiple,frame", GEOMETRIES)
def test_finish(shape, n, multiple, frame, elev_log, dtype):
    scenes = B.make_scenes([shape] * 3, seed=11)
    Sc = store(scenes, kinds=("lr_dem",), coord=None, elev_log=elev_log)
    _, fr = I.prepare(Sc, [0], n, multiple)
    (Hp, Wp), (H, W) = frame, shape
    g = torch.Generator().manual_seed(Hp * Wp + n)
    pred = torch.rand((3, 1, Hp, Wp), generator=g) * 1.6 - 0.3                # below 0 and above 1 as well
    special = [0.0, 1.0, float("nan"), -0.25, 1.5, -0.0]
    for b in range(3):
        for j, v in enumerate(special):                                       # inside the window, first and last rows
            pred[b, 0, n + (j % 2) * (H - 1), n + j] = v
    pred = pred.to(DEV).to(dtype)
    idx = [2, 0, 1]
    window = pred[:, 0, n:n + H, n:n + W]
    base = torch.tensor([float(np.float32(Sc.base[s])) for s in idx], dtype=torch.float32, device=DEV)
    assert len(set(base.tolist())) == 3
    n0 = launches(b"scene_finish")
    got = I.finish(pred, Sc, idx, fr, metres=True)
    assert launches(b"scene_finish") == n0 + 1
    want = M.descale_data(window.float().clamp(0.0, 1.0).contiguous(), Sc.elev_min, Sc.elev_max, elev_log) + base[:, None, None]
    assert got.dtype == torch.float32 and got.shape == (3, H, W)
    assert int(torch.isnan(got).sum()) == 3 and same(got, want)
    for b in range(3):                                                        # compose_scene's bits, one uncropped tile
        one = S.compose_scene(pred[b:b + 1, :, n:n + H, n:n + W].contiguous(), base[b], min(H, W), 0.0, Sc.elev_min, Sc.elev_max, elev_log)
        assert same(got[b], one)
    raw = I.finish(pred, Sc, idx, fr, metres=False)
    assert raw.dtype == torch.float32 and same(raw, window.float())


# ---- predict_scenes ------------------------------------------------------------------------------------------------------
IC = {"lr_dem": 1, "image": 3, "mask": 15}
SHAPES5 = [(40, 40), (37, 53), (40, 40), (37, 53), (40, 40)]


def jspsr_model(seed=5, ic=IC):
    from jspsr_amd.JSPSR import Model
    m = Model(dict(ic, COP30=1), num_feature=8)
    sd = O.make_state_dict(O.jspsr_param_shapes(ic, 8), seed=seed)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


@pytest.fixture(scope="module")
def five():
    scenes = B.make_scenes(SHAPES5, seed=21)
    Sc = store(scenes, kinds=("lr_dem", "image", "mask"), coord=None, hr=True)
    model, _ = jspsr_model()
    return scenes, Sc, model


def by_hand(model, Sc, idx, pad, metres=True):
    with torch.no_grad():
        inputs, fr = I.prepare(Sc, idx, pad, 8)
        return I.finish(model(*inputs), Sc, idx, fr, metres=metres)


def test_predict_scenes_batches_and_groups(five):
    scenes, Sc, model = five
    r3 = I.predict_scenes(model, Sc, batch_size=3, pad=4)
    assert r3.ids == Sc.ids and r3.shapes == SHAPES5 and r3.buffer.dtype == torch.float32 and r3.buffer.dim() == 1
    groups = {(40, 40): [0, 2, 4], (37, 53): [1, 3]}
    for (h, w), idx in groups.items():
        want = by_hand(model, Sc, idx, 4)
        for j, s in enumerate(idx):
            o = r3.offsets[s]
            assert torch.equal(r3.buffer[o:o + h * w].view(h, w), want[j]), s
    r1 = I.predict_scenes(model, Sc, batch_size=1, pad=4)
    for s, (h, w) in enumerate(SHAPES5):
        o = r1.offsets[s]
        assert torch.equal(r1.buffer[o:o + h * w].view(h, w), by_hand(model, Sc, [s], 4)[0]), s
    sub = I.predict_scenes(model, Sc, [3, 0], batch_size=2, pad=4)              # a subset, in the order named
    assert sub.ids == ["3", "0"] and sub.shapes == [(37, 53), (40, 40)]
    rasters = r3.rasters()
    assert list(rasters) == Sc.ids and [a.shape for a in rasters.values()] == SHAPES5
    assert all(a.dtype == np.float32 for a in rasters.values())
    assert torch.equal(sub.buffer[sub.offsets[0]:sub.offsets[0] + 37 * 53].view(37, 53), by_hand(model, Sc, [3], 4)[0])
    assert torch.equal(sub.buffer[sub.offsets[1]:sub.offsets[1] + 1600].view(40, 40), by_hand(model, Sc, [0], 4)[0])
    for s, (h, w) in enumerate(SHAPES5):
        o = r3.offsets[s]
        assert np.array_equal(rasters[str(s)], r3.buffer[o:o + h * w].view(h, w).cpu().numpy())
    a = S.summarise(Sc, list(rasters.values()), baselines={"COP30": "lr_dem"}, value_max=933, patch_size=128)
    b = S.summarise(Sc, [np.array(v, copy=True) for v in rasters.values()], baselines={"COP30": "lr_dem"}, value_max=933, patch_size=128)
    c = S.summarise(Sc, [r3.buffer[o:o + h * w].view(h, w) for o, (h, w) in zip(r3.offsets, r3.shapes)],
                    baselines={"COP30": "lr_dem"}, value_max=933, patch_size=128)
    assert a == b == c and set(a) == {"SR", "COP30"} and all(np.isfinite(v) for v in a["SR"].values())


def test_predict_scenes_bf16_model(five):
    scenes, Sc, model = five
    model.compute_dtype = torch.bfloat16
    try:
        r = I.predict_scenes(model, Sc, [0, 2, 4], batch_size=3, pad=4)
        want = by_hand(model, Sc, [0, 2, 4], 4)
    finally:
        model.compute_dtype = torch.float32
    assert torch.equal(r.buffer.view(3, 40, 40), want) and bool(torch.isfinite(r.buffer).all())
    lo, hi = Sc.elev_min + min(float(b) for b in Sc.base), Sc.elev_max + max(float(b) for b in Sc.base)
    assert lo <= float(r.buffer.min()) and float(r.buffer.max()) <= hi           # clamped, de-scaled, + base


def oracle_inputs(scene, p, n, multiple, kinds):
    ref = R.model_inputs({k: scene[k] for k in kinds}, p, n, multiple)
    return [torch.from_numpy(ref[k])[None].double() for k in kinds]


def close_to_oracle(got: np.ndarray, ref: torch.Tensor):
    ref = ref.detach().numpy()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"max |pred - oracle| = {err:.3e}, bound {1e-4 * np.abs(ref).max():.3e}")
    assert err < 1e-4 * np.abs(ref).max()                                       # tests/test_model_gpu.py: the fp32 eval forward


def test_jspsr_against_the_cpu_oracle():
    scenes = B.make_scenes([(40, 40)], seed=3)
    Sc = store(scenes, kinds=("lr_dem", "image", "mask"), coord=None)
    model, sd = jspsr_model(seed=9)
    r = I.predict_scenes(model, Sc, pad="pow2", metres=False)                   # cal_pad(40) = 12: a 64 x 64 frame
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        ref = O.jspsr_forward(sd64, oracle_inputs(scenes[0], params(), 12, 8, ("lr_dem", "image", "mask")), False)
    assert ref.shape == (1, 1, 64, 64)
    close_to_oracle(r.rasters()["0"], ref[0, 0, 12:52, 12:52])


def test_lrru_against_the_cpu_oracle():
    import types
    from jspsr_amd.LRRU import Model
    scenes = B.make_scenes([(40, 40)], seed=4)
    Sc = store(scenes, kinds=("lr_dem", "image"), coord=None)
    args = types.SimpleNamespace(input_channels={"lr_dem": 1, "image": 3}, output_channels=1, kernel_size=3, bc=16, prob=1.0,
                                 dkn_residual=True)
    m = Model(args)
    sd = O.make_state_dict(O.lrru_param_shapes(16), seed=12)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    r = I.predict_scenes(m, Sc, pad=1, metres=False)                            # 42 -> a 48 x 48 frame (multiple 16)
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        ref = O.lrru_forward(sd64, oracle_inputs(scenes[0], params(), 1, 16, ("lr_dem", "image")), False)
    assert ref.shape == (1, 1, 48, 48)
    close_to_oracle(r.rasters()["0"], ref[0, 0, 1:41, 1:41])


def test_edsr_concatenated_input_against_the_cpu_oracle():
    from jspsr_amd.EDSR import EDSR
    scenes = B.make_scenes([(37, 53)], seed=6)
    Sc = store(scenes, kinds=("lr_dem", "image"), coord=None)
    m = EDSR(in_channels=4, out_channels=1, n_resblocks=4, n_features=32, scale=1, spn=True)
    sd = O.make_state_dict(O.edsr_param_shapes(4, 4, 32), seed=13)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    r = I.predict_scenes(m, Sc, pad=5, metres=False, input_data={"lr_dem": 1, "image": 3})      # multiple 1: 47 x 63
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        ref = O.edsr_forward(sd64, torch.cat(oracle_inputs(scenes[0], params(), 5, 1, ("lr_dem", "image")), 1), False, n_resblocks=4)
    assert ref.shape == (1, 1, 47, 63)
    close_to_oracle(r.rasters()["0"], ref[0, 0, 5:42, 5:58])


# ---- upscale_dem ---------------------------------------------------------------------------------------------------------
def test_upscale_dem_keeps_the_reference_contract():
    scenes = B.make_scenes([(100, 100), (64, 64)], seed=8)
    model, _ = jspsr_model(seed=10)
    kw = {"min": -80, "max": 933, "log": True, "scale_mask": True}
    p = {"mask_channel": list(range(15)), "relative": True, "tensor_kwargs": kw, "model_name": "JSPSR", "input_data": IC}
    for s, pad, side in ((scenes[0], 14, 128), (scenes[1], 0, 64)):
        H = s["lr_dem"].shape[0]
        assert T.cal_pad(H, H) == pad
        sample = {"lr_dem": s["lr_dem"], "image": s["image"], "mask": s["mask"], "meta": {"id": "x", "base": np.min(s["lr_dem"])}}
        y, t_infer, m_infer = I.upscale_dem(model, sample, p)
        assert y.shape == (H, H, 1) and y.dtype == np.float32
        Sc = store([s], kinds=("lr_dem", "image", "mask"), coord=None)
        want = I.predict_scenes(model, Sc, pad="pow2", metres=False).rasters()["0"]
        assert np.array_equal(y[..., 0], want)
        assert np.array_equal(y[..., 0], by_hand(model, Sc, [0], pad, metres=False)[0].cpu().numpy())
        assert t_infer > 0
        assert m_infer * 1024 * 1024 >= side * side * 19 * 4                   # at least the inputs
    sample.pop("meta")
    with pytest.raises(KeyError):
        I.upscale_dem(model, sample, p)
    y, _, _ = I.upscale_dem(model, sample, dict(p, relative=False))             # absolute elevations need no meta
    assert y.shape == (64, 64, 1)


# ---- no host synchronisation -----------------------------------------------------------------------------------------------
def test_predict_scenes_does_not_synchronise(five, monkeypatch):
    scenes, Sc, model = five
    I.predict_scenes(model, Sc, [0, 2, 4], batch_size=2, pad=4)                 # warm: maps cached, weights packed
    calls = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self, *a, **k: calls.append("item") or 0)
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append("cpu") or real_cpu(self, *a, **k))
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        r = I.predict_scenes(model, Sc, [0, 2, 4], batch_size=2, pad=4)         # two batches
        stop.record()
    assert calls == []
    monkeypatch.undo()
    stream.synchronize()
    rasters = r.rasters()
    assert start.elapsed_time(stop) > 0 and len(rasters) == 3
    want = I.predict_scenes(model, Sc, [0, 2, 4], batch_size=2, pad=4).rasters()
    assert all(np.array_equal(rasters[k], want[k]) for k in want)
