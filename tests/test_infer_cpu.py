"""Whole-scene inference without a GPU: `infer.frame_maps` against `tiles.add_padding` and against the arrays the
reference's own add_padding / remove_padding / cal_pad / scale_data produced (tests/golden/g14_infer.npz,
tools/gen_golden_infer.py); the restatement tests/infer_ref.py against the same arrays; `InferenceScenes`' upload checks;
`upscale_dem`'s refusal of a frame its model cannot take.  Everything here is compared with ==."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from jspsr_amd import infer as I
from jspsr_amd import tiles as T
from tests import batches_ref as B
from tests import infer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(40, 40, 12), (37, 53, 5), (9, 7, 6), (100, 100, 14)]


@pytest.fixture(scope="module")
def g14(golden_dir):
    z = np.load(os.path.join(golden_dir, "g14_infer.npz"))
    assert int(z["seed"]) == R.SEED and str(z["inputs_checksum"]) == R.inputs_checksum(), \
        "fixture inputs do not regenerate: rerun tools/gen_golden_infer.py"
    return z


def generator():
    spec = importlib.util.spec_from_file_location("gen_golden_infer", os.path.join(ROOT, "tools", "gen_golden_infer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gather(a, rows, cols):
    return a[rows.astype(np.int64)][:, cols.astype(np.int64)]


@pytest.mark.parametrize("H,W,n", GEOMETRIES)
def test_frame_maps_reproduce_add_padding_on_index_rasters(H, W, n):
    rows, cols, top, left = I.frame_maps(H, W, n, 1)
    assert rows.dtype == cols.dtype == np.int32 and (top, left) == (n, n)
    x = torch.arange(2 * H * W, dtype=torch.float32).reshape(2, H, W)
    want = T.add_padding(x, n).numpy()
    assert np.array_equal(x.numpy()[:, rows.astype(np.int64)][:, :, cols.astype(np.int64)], want)
    hwc = np.ascontiguousarray(x.numpy().transpose(1, 2, 0))
    assert np.array_equal(R.add_padding(hwc, n), want.transpose(1, 2, 0))
    assert np.array_equal(R.frame(hwc, n, 1), want.transpose(1, 2, 0))


def test_maps_tiles_and_restatement_against_the_reference_made_arrays(g14):
    arrays, _ = R.golden_inputs()
    for i, (a, (H, W, C, n)) in enumerate(zip(arrays, R.PAD_CASES)):
        want = g14[f"pad{i}"]
        assert want.shape == (H + 2 * n, W + 2 * n, C) and want.dtype == np.float32
        rows, cols, _, _ = I.frame_maps(H, W, n, 1)
        assert np.array_equal(gather(a, rows, cols).astype(np.float32), want), i
        assert np.array_equal(R.add_padding(a, n), want), i
        chw = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32))
        padded = T.add_padding(chw, n)
        assert np.array_equal(padded.numpy().transpose(1, 2, 0), want), i
        assert np.array_equal(T.remove_padding(padded, n).numpy().transpose(1, 2, 0), g14[f"unpad{i}"]), i
        assert np.array_equal(R.remove_padding(want, n), g14[f"unpad{i}"]) and np.array_equal(g14[f"unpad{i}"], a.astype(np.float32))
    assert [T.cal_pad(s, s) for s in R.CAL_PAD_SIDES] == list(g14["cal_pad"])
    assert list(g14["cal_pad"]) == [13, 12, 14, 89, 0, 0, 0]


def test_scale_data_restatement_against_the_reference_made_arrays(g14):
    _, dem = R.golden_inputs()
    padded = R.add_padding(dem, R.DEM_PAD)
    for log in (True, False):
        for with_base in (True, False):
            p = {"elev_log": log, "elev_min": R.ELEV_MIN, "elev_max": R.ELEV_MAX}
            got = B.scale_dem(padded, p, float(np.min(dem)) if with_base else 0)
            want = g14[f"scale_{'log' if log else 'lin'}_{'base' if with_base else 'nobase'}"]
            assert got.dtype == want.dtype and np.array_equal(got, want), (log, with_base)
            assert want.min() >= 0 and want.max() <= 1


def test_fixture_regenerates_from_the_reference(g14):
    """With the reference tree at hand every array is made again by its own functions and compared bit for bit; without
    it the inputs' checksum (the g14 fixture above) is what holds the fixture to its seed."""
    gen = generator()
    if not gen.reference_available():
        return
    again = gen.generate()
    assert sorted(again) == sorted(g14.files)
    for k, v in again.items():
        assert np.asarray(v).dtype == g14[k].dtype and np.array_equal(np.asarray(v), g14[k]), k


def test_frames_brought_to_a_multiple():
    rows, cols, top, left = I.frame_maps(37, 53, 5, 8)
    assert (len(rows), len(cols), top, left) == (48, 64, 5, 5)
    assert list(rows[-3:]) == [32, 31, 30] and list(rows[42:45]) == [35, 34, 33]      # the border's last rows, then on
    assert list(cols[58:]) == [52, 51, 50, 49, 48, 47]
    r0, c0, _, _ = I.frame_maps(37, 53, 5, 1)
    assert np.array_equal(rows[:47], r0) and np.array_equal(cols[:63], c0)            # the extension changes nothing before it
    rows, cols, top, left = I.frame_maps(37, 53, 0, 8)
    assert (len(rows), len(cols), top, left) == (40, 56, 0, 0)
    assert list(rows[:37]) == list(range(37)) and list(rows[37:]) == [35, 34, 33] and list(cols[53:]) == [52, 51, 50]
    a = np.arange(37 * 53 * 2, dtype=np.float32).reshape(37, 53, 2)
    for n, m in ((5, 8), (0, 8), (5, 16), (3, 1)):
        rows, cols, _, _ = I.frame_maps(37, 53, n, m)
        assert np.array_equal(gather(a, rows, cols), R.frame(a, n, m)), (n, m)
        assert rows.min() >= 0 and rows.max() < 37 and cols.min() >= 0 and cols.max() < 53


@pytest.mark.parametrize("H,W,n,m", [(5, 20, 6, 1),          # n <= H
                                     (9, 20, 9, 1), (10, 40, 5, 16),      # n + eh <= H - 1
                                     (20, 7, 8, 1), (40, 10, 5, 16)])     # n + ew <= W
def test_frame_maps_refuse_what_the_scene_cannot_fill(H, W, n, m):
    with pytest.raises(ValueError):
        I.frame_maps(H, W, n, m)


def test_frame_maps_at_the_validity_limits():
    rows, cols, _, _ = I.frame_maps(9, 20, 8, 1)
    assert rows.min() == 0 and rows[-1] == 0 and rows.max() == 8
    rows, cols, _, _ = I.frame_maps(20, 7, 7, 1)
    assert cols.min() == 0 and cols[-1] == 0 and cols[0] == 6


def host_scenes(scenes, **kw):
    p = {k: v for k, v in dict(B.PARAMS, **kw).items() if k != "label_range"}
    kinds = {k: [s[k] for s in scenes] for k in ("lr_dem", "image", "mask", "canopy") if k in scenes[0]}
    return I.InferenceScenes(**kinds, device="cpu", **p)


def test_inference_scenes_checks_and_members():
    scenes = B.make_scenes([(40, 40), (36, 30)])
    S = host_scenes(scenes)
    assert "hr_dem" not in S.store and S.kinds == ["lr_dem", "image", "mask", "canopy"]
    assert S.base == [np.min(s["lr_dem"]) for s in scenes] and S.shapes == [(40, 40), (36, 30)] and S.ids == ["0", "1"]
    assert S.scene_table.tolist() == [[0, 40, 40], [1600, 36, 30]] and S.channels == {"lr_dem": 1, "image": 3, "mask": 15, "canopy": 1}
    assert S.store["mask"].numel() == (1600 + 1080) * 15 and S.store["lr_dem"].dtype == torch.float32
    assert host_scenes(scenes, relative=False, elev_min=0, elev_max=1000).base == [0, 0]
    full = {k: [s[k] for s in scenes] for k in ("lr_dem", "hr_dem", "image", "mask", "canopy")}
    from jspsr_amd import data as D
    ref = D.DeviceScenes(**full, device="cpu", **B.PARAMS)
    assert ref.flags == S.flags and ref.base == S.base and torch.equal(ref.scene_table, S.scene_table)
    for k in S.store:
        assert torch.equal(ref.store[k], S.store[k])
    bad = [dict(s) for s in scenes]
    bad[0]["lr_dem"] = bad[0]["lr_dem"].astype(np.float64)
    with pytest.raises(ValueError):                                 # wrong dtype
        host_scenes(bad)
    bad = [dict(s) for s in scenes]
    bad[1]["mask"] = bad[1]["mask"][..., :14]
    with pytest.raises(ValueError):                                 # channel mismatch
        host_scenes(bad)
    bad = [dict(s) for s in scenes]
    bad[1]["image"] = bad[1]["image"][:-1]
    with pytest.raises(ValueError):                                 # a raster of another size
        host_scenes(bad)
    with pytest.raises(AssertionError):
        host_scenes(scenes, relative=False, elev_max=300)           # scaled values above 1
    bad = [dict(s) for s in scenes]
    bad[1]["lr_dem"] = bad[1]["lr_dem"].copy()
    bad[1]["lr_dem"][3, 4, 0] = -100.0
    with pytest.raises(AssertionError):                             # log domain broken
        host_scenes(bad, relative=False)
    with pytest.raises(NotImplementedError):
        host_scenes(scenes, coord="global")


def test_upscale_dem_refuses_a_frame_that_is_no_multiple():
    from jspsr_amd.JSPSR import Model
    from jspsr_amd.LRRU import Model as LRRU
    from jspsr_amd.EDSR import EDSR
    assert (Model.size_multiple, LRRU.size_multiple, EDSR.size_multiple) == (8, 16, 1)
    model = Model({"lr_dem": 1, "image": 3, "COP30": 1}, num_feature=8)
    s = B.make_scenes([(37, 37)])[0]
    p = {"mask_channel": None, "relative": False, "tensor_kwargs": {"min": -80, "max": 933, "log": True}, "model_name": "JSPSR",
         "input_data": {"lr_dem": 1, "image": 3}}
    assert T.cal_pad(37, 37) == 13                                  # a 63-pixel frame
    with pytest.raises(ValueError, match="predict_scenes"):
        I.upscale_dem(model, {"lr_dem": s["lr_dem"], "image": s["image"]}, p)


def test_entries_refuse_bad_arguments_before_any_launch():
    """Argument checks return JSPSR_EINVAL before a launch (safe without a GPU; the pointers are never dereferenced)."""
    import ctypes
    from jspsr_amd import _lib
    lib = _lib.load()
    x = ctypes.c_void_p(4096)
    finish = lambda *a: lib.jspsr_scene_finish(*a, 1, 1, -80.0, 933.0, None)      # noqa: E731
    assert finish(0, None, x, x, 1, 64, 64, 12, 12, 40, 40) == -1 and b"scene_finish" in lib.jspsr_last_error()
    assert finish(0, x, x, x, 0, 64, 64, 12, 12, 40, 40) == -1                      # B <= 0
    assert finish(0, x, x, x, 1, 64, 64, 25, 12, 40, 40) == -1 and b"leaves" in lib.jspsr_last_error()
    assert finish(0, x, x, x, 1, 64, 64, 12, -1, 40, 40) == -1
    assert finish(0, x, x, x, 1, 64, 64, 12, 12, 40, 53) == -1
    assert finish(2, x, x, x, 1, 64, 64, 12, 12, 40, 40) == -1                      # neither fp32 nor bf16
    six_p, six_ll, six_i = ctypes.c_void_p * 6, ctypes.c_longlong * 6, ctypes.c_int * 6
    src, nbytes, out = six_p(), six_ll(), six_p()
    ch, coff, pitch = six_i(), six_i(), six_i()

    def prepare(B=1, Hp=64, Wp=64, rows=x, mask_div=16, flags=0):
        return lib.jspsr_scene_prepare(src, nbytes, out, ch, coff, pitch, x, 1, x, B, rows, x, Hp, Wp, flags, -80.0, 933.0, mask_div, None)

    assert prepare() == -1 and b"no output" in lib.jspsr_last_error()
    assert prepare(B=0) == -1 and prepare(Hp=0) == -1 and prepare(rows=None) == -1 and prepare(mask_div=0) == -1 and prepare(flags=64) == -1
    out[1], ch[1], pitch[1] = 4096, 1, 1                                            # hr_dem is no input
    assert prepare() == -1 and b"hr_dem" in lib.jspsr_last_error()
    out[1] = None
    out[3], ch[3], pitch[3] = 4096, 17, 17                                          # more channels than a kind takes
    assert prepare() == -1
    ch[3], pitch[3] = 15, 14                                                        # pitch smaller than the channels
    assert prepare() == -1
    ch[3], pitch[3] = 15, 15                                                        # a kind without its store
    assert prepare() == -1 and b"store" in lib.jspsr_last_error()
