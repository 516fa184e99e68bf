"""K14 on the MI355X: jspsr_scene_prepare_d4 / jspsr_scene_finish_mean and `predict_scenes(tta=...)` against an oracle put
together from what K13 already gives: the raw numpy rasters transformed with np.rot90 / fliplr / flipud, a fresh
`InferenceScenes` of them, K13's `prepare` / `finish` / `predict_scenes(metres=False)`, the transform undone in numpy, the
variants added one after the other in fp32 and divided by fp32(K) in numpy (a true division; torch divides a device tensor
by a Python number through its reciprocal).

Bound: none.  Every comparison is bit for bit (`view(int32)`, NaN included): the index maps are integers, the per-kind
arithmetic is the shared csrc/totensor.h, and the mean is a fixed sequence of fp32 operations.

coord.  A transformed store with coord="local" would hold the coordinates of the TRANSFORMED pixel; the self-ensemble
transforms coord with the other rasters, so that a pixel keeps the local coordinates of its SOURCE pixel (as the
reference's augmentation rotates sample["coord"]).  Its oracle is therefore K13's coord planes of the untransformed store,
transformed and padded on the host; every other kind is compared with `prepare` on the transformed store directly."""
import functools

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import infer as I
from tests import batches_ref as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# scene (H, W), pad, multiple -> the frames of the two rot90 parities
GEOMETRIES = [((13, 10), 3, 8, (24, 16), (16, 24)),          # W % 4 != 0, both extensions non-zero
              ((16, 12), 0, 4, (16, 12), (12, 16)),          # 16-byte stores
              ((9, 9), 2, 1, (13, 13), (13, 13))]            # square, odd
GEOMETRY_IDS = ["13x10", "16x12", "9x9"]
KINDS = ("lr_dem", "image", "mask", "coord")
ELEMENT_SETS = {1: [(0, False, False)], 2: [(1, True, False), (0, False, True)], 3: [(3, False, False), (0, True, False), (1, False, True)],
                8: I.d4_elements("d4")}


def launches(name):
    return _lib.load().jspsr_launch_count(name)


def bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and torch.equal(a, b)


def params(**kw):
    return {k: v for k, v in dict(B.PARAMS, **kw).items() if k != "label_range"}


def store(scenes, kinds=("lr_dem", "image", "mask"), coord="local", base=None, **kw):
    return I.InferenceScenes(coord=coord, device=DEV, base=base, **{k: [s[k] for s in scenes] for k in kinds}, **params(**kw))


def transformed(scenes, element, kinds=("lr_dem", "image", "mask")):
    return [{k: np.ascontiguousarray(I.d4_apply(s[k], element)) for k in kinds} for s in scenes]


@functools.lru_cache(maxsize=None)
def two_scenes(shape, elev_log):
    """Two scenes with lr_dem, image (3 channels) and a mask of 2 selected channels (scale_mask), coord "local",
    relative=True -> (raw scenes, their store, K13's unpadded coord planes (2, 2, H, W) of scenes 1, 0 of that store)."""
    scenes = B.make_scenes([shape] * 2, seed=shape[0] * 31 + shape[1], mask_c=2)
    Sc = store(scenes, mask_channel=[0, 1], elev_log=elev_log)
    plain, _ = I.prepare(Sc, [1, 0], 0, 1)
    return scenes, Sc, plain[3].cpu().numpy()                                  # coord (2, 2, H, W), scenes 1, 0


@functools.lru_cache(maxsize=None)
def oracle_inputs(shape, elev_log, pad, multiple, code):
    """K13 on a store of the transformed rasters, scenes [1, 0]: {kind: (2, C, Hp, Wp) tensor}; coord as the module's
    docstring says."""
    scenes, Sc, coord = two_scenes(shape, elev_log)
    St = store(transformed(scenes, code), mask_channel=[0, 1], elev_log=elev_log, base=list(Sc.base))
    assert [float(a) for a in St.base] == [float(a) for a in Sc.base]
    inputs, frame = I.prepare(St, [1, 0], pad, multiple)
    out = dict(zip(KINDS, inputs))
    t = I.d4_apply(coord, code, axes=(2, 3))
    rows, cols, _, _ = I.frame_maps(t.shape[2], t.shape[3], pad, multiple)
    out["coord"] = torch.from_numpy(np.ascontiguousarray(t[:, :, rows.astype(np.int64)][:, :, :, cols.astype(np.int64)])).to(DEV)
    if code == 0:                                                               # the identity: K13's own coord, bit for bit
        assert same_bits(out["coord"], inputs[3])
    return out, frame


def split(inputs, Sc, concat):
    if not concat:
        return dict(zip(KINDS, inputs))
    out, c0 = {}, 0
    for k in KINDS:
        out[k] = inputs[0][:, c0:c0 + Sc.channels[k]]
        c0 += Sc.channels[k]
    assert c0 == inputs[0].shape[1] == 8
    return out


# ---- 1. prepare_d4 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("elev_log", [True, False])
@pytest.mark.parametrize("shape,pad,multiple,even,odd", GEOMETRIES, ids=GEOMETRY_IDS)
def test_prepare_d4_bit_for_bit(shape, pad, multiple, even, odd, elev_log, concat):
    scenes, Sc, _ = two_scenes(shape, elev_log)
    for ud in (False, True):                                                    # 2 x 8 distinct elements: all 16 codes
        elements = [(r, lr, ud) for r in range(4) for lr in (False, True)]
        n0 = launches(b"scene_prepare_d4")
        groups = I.prepare_d4(Sc, [1, 0], elements, pad, multiple, concat=concat)
        assert launches(b"scene_prepare_d4") == n0 + 2 and sorted(groups) == [0, 1]
        for parity, (inputs, frame, order) in groups.items():
            h, w = shape[::-1] if parity else shape
            assert (frame.Hp, frame.Wp) == (odd if parity else even) and (frame.top, frame.left, frame.H, frame.W) == (pad, pad, h, w)
            assert [e for _, e in order[::2]] == [e for e in elements if e[0] % 2 == parity] and [j for j, _ in order] == [0, 1] * 4
            assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == 8 for t in inputs)
            got = split(inputs, Sc, concat)
            for j, (_, e) in enumerate(order[::2]):
                want, fr = oracle_inputs(shape, elev_log, pad, multiple, I.d4_code(e))
                assert fr == frame
                for kind in KINDS:
                    g = got[kind][2 * j:2 * j + 2]
                    assert not bool(torch.isnan(g).any())
                    assert same_bits(g, want[kind]), (e, kind, (bits(g) != bits(want[kind])).nonzero()[:4].tolist())


def test_prepare_d4_mixes_even_codes_in_one_launch():
    shape, pad, multiple = (13, 10), 3, 8
    scenes, Sc, _ = two_scenes(shape, True)
    elements = [(2, True, False), (0, False, False), (2, False, False), (0, True, False)]
    n0 = launches(b"scene_prepare_d4")
    groups = I.prepare_d4(Sc, [1, 0], elements, pad, multiple)
    assert launches(b"scene_prepare_d4") == n0 + 1 and list(groups) == [0]
    inputs, frame, order = groups[0]
    assert [e for _, e in order[::2]] == elements
    for j, e in enumerate(elements):
        want, _ = oracle_inputs(shape, True, pad, multiple, I.d4_code(e))
        for kind, t in zip(KINDS, inputs):
            assert same_bits(t[2 * j:2 * j + 2], want[kind]), (e, kind)
    # the raw call: a device table whose code disagrees with the launch's parity, or names no scene, gives NaN samples
    rows, cols, _ = I._device_maps(13, 10, pad, multiple, Sc.device)
    base = int(np.float32(Sc.base[0]).view(np.int32))
    table = torch.tensor([[0, base, 0], [0, base, 4], [5, base, 0], [0, base, 16]], dtype=torch.int32, device=DEV)
    out = torch.full((4, 1, 24, 16), -7.0, device=DEV)
    I.launch_prepare_d4(Sc, table, [0, 0, 0, 0], rows, cols, 24, 16, {"lr_dem": (out, 0)})
    want, _ = oracle_inputs(shape, True, pad, multiple, 0)
    assert same_bits(out[0], want["lr_dem"][1]) and bool(torch.isnan(out[1:]).all())


@pytest.mark.parametrize("guard", [5, 8])
@pytest.mark.parametrize("shape,pad,multiple,even,odd", GEOMETRIES[:2], ids=GEOMETRY_IDS[:2])
def test_prepare_d4_writes_nothing_outside_its_channels(shape, pad, multiple, even, odd, guard):
    """The odd-parity launch into channel slices of a larger tensor filled with a sentinel, one spare channel either side of
    each sample, `guard` elements into the allocation (5: no 16-byte alignment; 8: aligned)."""
    scenes, Sc, _ = two_scenes(shape, True)
    elements = [(1, False, False), (3, True, False)]
    want = I.prepare_d4(Sc, [1, 0], elements, pad, multiple, concat=True)[1][0][0]
    (Hp, Wp), C = odd, 8
    numel = 4 * (C + 2) * Hp * Wp
    big = torch.full((numel + 2 * guard,), -7.0, device=DEV)
    view = big[guard:guard + numel].view(4, C + 2, Hp, Wp)
    outs, c0 = {}, 1
    for k in KINDS:
        outs[k] = (view, c0)
        c0 += Sc.channels[k]
    rows, cols, _ = I._device_maps(shape[1], shape[0], pad, multiple, Sc.device)
    table, host = I._table_d4(Sc, [1, 0], [4, 14])
    I.launch_prepare_d4(Sc, table, host, rows, cols, Hp, Wp, outs)
    assert same_bits(view[:, 1:C + 1], want)
    assert bool((view[:, 0] == -7.0).all()) and bool((view[:, C + 1] == -7.0).all())
    assert bool((big[:guard] == -7.0).all()) and bool((big[guard + numel:] == -7.0).all())


# ---- 2. finish_mean ------------------------------------------------------------------------------------------------------
def host_mean(windows, elements):
    """windows[k] (B, h_k, w_k) fp32 numpy -> the inverse transforms, added in order in fp32, divided by fp32(K)."""
    acc = None
    for y, e in zip(windows, elements):
        y = np.ascontiguousarray(I.d4_invert(y, e, axes=(1, 2)), dtype=np.float32)
        acc = y if acc is None else (acc + y).astype(np.float32)
    return (acc / np.float32(len(elements))).astype(np.float32)


def in_metres(mean, Sc, idx, metres):
    """K13's finish on the mean as a prediction whose frame is the scene: scene_finish_kernel's own expressions."""
    t = torch.from_numpy(mean).to(DEV)
    h, w = mean.shape[1:]
    return I.finish(t[:, None], Sc, idx, I.Frame(h, w, 0, 0, h, w), metres=metres)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("elev_log", [True, False])
@pytest.mark.parametrize("shape,pad,multiple,even,odd", GEOMETRIES, ids=GEOMETRY_IDS)
def test_finish_mean_bit_for_bit(shape, pad, multiple, even, odd, elev_log, dtype):
    scenes, Sc, _ = two_scenes(shape, elev_log)
    H, W = shape
    idx = [1, 0]
    frames = {0: I.Frame(*even, pad, pad, H, W), 1: I.Frame(*odd, pad, pad, W, H)}
    g = torch.Generator().manual_seed(H * 100 + W + pad)
    for K, elements in ELEMENT_SETS.items():
        preds = []
        for k, e in enumerate(elements):
            f = frames[e[0] % 2]
            p = torch.rand((2, 1, f.Hp, f.Wp), generator=g) * 1.6 - 0.3         # below 0 and above 1 as well
            p[0, 0, pad + 1, pad + 2] = -0.0
            if k == min(1, K - 1):
                p[1, 0, pad + f.H - 1, pad] = float("nan")                      # one NaN, in one variant
            preds.append(p.to(DEV).to(dtype))
        windows = [I.finish(p, Sc, idx, frames[e[0] % 2], metres=False).cpu().numpy() for p, e in zip(preds, elements)]
        mean = host_mean(windows, elements)
        assert int(np.isnan(mean).sum()) == 1
        if K == 1:
            assert (mean[np.isfinite(mean)] < 0).any() and (mean[np.isfinite(mean)] > 1).any()
        for metres in (False, True):
            n0 = launches(b"scene_finish_mean")
            got = I.finish_mean(preds, Sc, idx, frames, elements, metres=metres)
            assert launches(b"scene_finish_mean") == n0 + 1
            assert got.dtype == torch.float32 and got.shape == (2, H, W) and int(torch.isnan(got).sum()) == 1
            want = in_metres(mean, Sc, idx, metres)
            assert same_bits(got, want), (K, metres, (bits(got) != bits(want)).nonzero()[:4].tolist())
            if K == 1:                                                          # the identity alone: K13's finish on the same tensor
                assert same_bits(got, I.finish(preds[0], Sc, idx, frames[0], metres=metres))
            per_frame = I.finish_mean(preds, Sc, idx, [frames[e[0] % 2] for e in elements], elements, metres=metres)
            assert same_bits(per_frame, got)


# ---- 3. end to end, a stub whose output depends on the position ------------------------------------------------------------
class Stub(torch.nn.Module):
    """Not equivariant under any flip or turn: the ramp is tied to the frame, so a wrong inverse or window shows."""
    size_multiple = 8

    def forward(self, lr_dem, image):
        Hp, Wp = lr_dem.shape[2:]
        Y = torch.arange(Hp, dtype=torch.float32, device=lr_dem.device)[:, None]
        X = torch.arange(Wp, dtype=torch.float32, device=lr_dem.device)[None, :]
        return lr_dem * 0.75 + image.mean(1, keepdim=True) * 0.5 + (Y * 0.03125 - X * 0.0078125)


def oracle_ensemble(model, scenes, Sc, elements, pad, kinds, **kw):
    """Per scene: K13 on a one-scene store of each transformed sample -> the inverse -> the fp32 mean."""
    out = []
    for s, sc in enumerate(scenes):
        windows = []
        for e in elements:
            St = store(transformed([sc], e, kinds), kinds=kinds, coord=None, base=[Sc.base[s]])
            windows.append(I.predict_scenes(model, St, pad=pad, metres=False, **kw).rasters()["0"][None])
        out.append(host_mean(windows, elements))
    return out


@pytest.mark.parametrize("batch_size", [3, 16])
def test_predict_scenes_tta_with_a_position_dependent_stub(batch_size):
    shapes = [(13, 10), (9, 9), (13, 10)]
    scenes = B.make_scenes(shapes, seed=41)
    kinds = ("lr_dem", "image")
    Sc = store(scenes, kinds=kinds, coord=None)
    model = Stub().to(DEV)
    elements = I.d4_elements("d4")
    kw = dict(model_name="jspsr")
    want = oracle_ensemble(model, scenes, Sc, elements, 3, kinds, **kw)
    assert not np.array_equal(want[0], I.predict_scenes(model, Sc, [0], pad=3, metres=False, **kw).rasters()["0"][None])
    for metres in (False, True):
        n0 = launches(b"scene_finish_mean"), launches(b"scene_finish")
        r = I.predict_scenes(model, Sc, batch_size=batch_size, pad=3, metres=metres, tta="d4", **kw)
        assert launches(b"scene_finish") == n0[1] and launches(b"scene_finish_mean") > n0[0]
        assert r.ids == Sc.ids and r.shapes == shapes
        for s, (h, w) in enumerate(shapes):
            got = r.buffer[r.offsets[s]:r.offsets[s] + h * w].view(1, h, w)
            assert same_bits(got, in_metres(want[s], Sc, [s], metres)), (batch_size, metres, s)
        one = I.predict_scenes(model, Sc, batch_size=batch_size, pad=3, metres=metres, tta=[(0, False, False)], **kw)
        none = I.predict_scenes(model, Sc, batch_size=batch_size, pad=3, metres=metres, **kw)
        assert one.offsets == none.offsets and same_bits(one.buffer, none.buffer)
    sub = I.predict_scenes(model, Sc, [2, 1], batch_size=batch_size, pad=3, metres=False, tta=[(1, False, False), (0, True, False), 10], **kw)
    want3 = oracle_ensemble(model, [scenes[2], scenes[1]], store([scenes[2], scenes[1]], kinds=kinds, coord=None),
                            [(1, False, False), (0, True, False), (2, True, False)], 3, kinds, **kw)
    for j, (h, w) in enumerate([(13, 10), (9, 9)]):
        assert same_bits(sub.buffer[sub.offsets[j]:sub.offsets[j] + h * w].view(1, h, w), want3[j])
    with pytest.raises(ValueError, match="same element"):
        I.predict_scenes(model, Sc, pad=3, tta=[0, 11], **kw)


def test_predict_scenes_tta_does_not_synchronise(monkeypatch):
    scenes = B.make_scenes([(13, 10), (13, 10)], seed=43)
    Sc = store(scenes, kinds=("lr_dem", "image"), coord=None)
    model = Stub().to(DEV)
    want = I.predict_scenes(model, Sc, batch_size=8, pad=3, tta="d4", model_name="jspsr").buffer.clone()   # warm: tables cached
    uploads = len(Sc._infer_tables), len(I._MAPS)
    calls = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self, *a, **k: calls.append("item") or 0)
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append("cpu") or self)
    r = I.predict_scenes(model, Sc, batch_size=8, pad=3, tta="d4", model_name="jspsr")
    monkeypatch.undo()
    assert calls == [] and (len(Sc._infer_tables), len(I._MAPS)) == uploads     # nothing uploaded again either
    assert same_bits(r.buffer, want)


# ---- 4. end to end, a real model --------------------------------------------------------------------------------------------
def test_predict_scenes_tta_with_jspsr():
    from jspsr_amd.JSPSR import Model
    from oracle import jspsr_ref as O
    ic = {"lr_dem": 1, "image": 3, "mask": 15}
    model = Model(dict(ic, COP30=1), num_feature=8)
    model.load_state_dict(O.make_state_dict(O.jspsr_param_shapes(ic, 8), seed=5))
    model = model.to(DEV).eval()
    scenes = B.make_scenes([(40, 24)] * 2, seed=47)
    Sc = store(scenes, coord=None)
    elements = I.d4_elements("d4")
    r = I.predict_scenes(model, Sc, batch_size=16, pad=4, metres=False, tta="d4")
    # the oracle's per-variant predictions: the model on the very tensors prepare_d4 returns (test 1: K13's bits on the
    # transformed store), in the same batch composition
    windows = {}
    with torch.no_grad():
        groups = I.prepare_d4(Sc, [0, 1], elements, 4, 8)
        assert {p: (f.Hp, f.Wp) for p, (_, f, _) in groups.items()} == {0: (48, 32), 1: (32, 48)}
        for parity, (inputs, frame, order) in groups.items():
            pred = model(*inputs)
            assert pred.shape == (8, 1, frame.Hp, frame.Wp) and pred.dtype == torch.float32
            for j, (_, e) in enumerate(order[::2]):
                windows[e] = I.finish(pred[2 * j:2 * j + 2], Sc, [0, 1], frame, metres=False).cpu().numpy()
    want = host_mean([windows[e] for e in elements], elements)
    assert np.isfinite(want).all()
    assert same_bits(r.buffer.view(2, 40, 24), want)
    single = I.predict_scenes(model, Sc, batch_size=16, pad=4, metres=False)
    assert not torch.equal(single.buffer, r.buffer)                              # the ensemble did something
    metres = I.predict_scenes(model, Sc, batch_size=16, pad=4, tta="d4")
    assert same_bits(metres.buffer.view(2, 40, 24), in_metres(want, Sc, [0, 1], True))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_and_launch_nothing():
    shape, pad, multiple = (13, 10), 3, 8
    scenes, Sc, _ = two_scenes(shape, True)
    even, odd = I.Frame(24, 16, 3, 3, 13, 10), I.Frame(16, 24, 3, 3, 10, 13)
    pe, po = torch.zeros((2, 1, 24, 16), device=DEV), torch.zeros((2, 1, 16, 24), device=DEV)
    idx = [1, 0]
    n0 = launches(b"scene_finish_mean"), launches(b"scene_prepare_d4")

    def refused(what, match, call, *a, **k):
        with pytest.raises(_lib.JspsrHipError, match=match) as err:
            call(*a, **k)
        assert what in str(err.value) and "code -1" in str(err.value)

    fin = "jspsr_scene_finish_mean"
    refused(fin, "0 variants", I.finish_mean, [], Sc, idx, [], [])
    nine = [pe.clone() for _ in range(9)]
    refused(fin, "9 variants", I.finish_mean, nine, Sc, idx, [even] * 9, [0, 2, 8, 10, 1, 3, 9, 11, 0])
    refused(fin, "same element", I.finish_mean, [pe, pe], Sc, idx, [even, even], [0, 11])
    refused(fin, "same element", I.finish_mean, [po, pe, po], Sc, idx, [odd, even, odd], [(1, False, False), 0, (3, True, True)])
    refused(fin, "leaves", I.finish_mean, [pe], Sc, idx, [I.Frame(24, 16, 12, 3, 13, 10)], [0])
    refused(fin, "leaves", I.finish_mean, [po], Sc, idx, [I.Frame(16, 24, 3, 12, 10, 13)], [4])
    refused(fin, "transforms to 10 x 13", I.finish_mean, [pe], Sc, idx, [even], [4])          # a quarter turn in the upright frame
    refused(fin, "transforms to 13 x 10", I.finish_mean, [po], Sc, idx, [odd], [0])
    with pytest.raises(ValueError, match="finish_mean"):                                     # the tensor is not the frame's
        I.finish_mean([pe], Sc, idx, [odd], [4])

    prep = "jspsr_scene_prepare_d4"
    rows, cols, _ = I._device_maps(13, 10, pad, multiple, Sc.device)
    out = torch.full((2, 1, 24, 16), -7.0, device=DEV)
    table = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    refused(prep, "one parity", I.launch_prepare_d4, Sc, table, [0, 4], rows, cols, 24, 16, {"lr_dem": (out, 0)})
    refused(prep, "one parity", I.launch_prepare_d4, Sc, table, [14, 10], rows, cols, 24, 16, {"lr_dem": (out, 0)})
    refused(prep, "outside 0..15", I.launch_prepare_d4, Sc, table, [0, 16], rows, cols, 24, 16, {"lr_dem": (out, 0)})
    refused(prep, "no output", I.launch_prepare_d4, Sc, table, [0, 0], rows, cols, 24, 16, {})
    assert (launches(b"scene_finish_mean"), launches(b"scene_prepare_d4")) == n0 and bool((out == -7.0).all())
    lib = _lib.load()                                                                         # the codes, as they come back
    assert lib.jspsr_scene_finish_mean((_lib.TtaVariant * 1)(), 0, out.data_ptr(), table.data_ptr(), 2, 13, 10, 1, 1, -80.0, 933.0, None) == -1
    assert lib.jspsr_scene_finish_mean((_lib.TtaVariant * 1)(_lib.TtaVariant(pe.data_ptr() + 2, 0, 0, 24, 16, 3, 3, 13, 10)), 1,
                                       out.data_ptr(), table.data_ptr(), 2, 13, 10, 1, 1, -80.0, 933.0, None) == -2
    with pytest.raises(ValueError, match=r"frame_maps: element \(1, False, False\)"):         # 12 x 4, border 4: upright only
        I.prepare_d4(store(B.make_scenes([(12, 4)], seed=3, mask_c=2), mask_channel=[0, 1]), [0], [(1, False, False)], 4, 1)
    assert (launches(b"scene_finish_mean"), launches(b"scene_prepare_d4")) == n0
