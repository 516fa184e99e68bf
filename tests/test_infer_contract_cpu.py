"""Whole-scene inference without a GPU, the refusals around the stores and `upscale_dem`: a `DeviceScenes` still needs its
ground truth (only `InferenceScenes` is a store without one); `upscale_dem` names what is missing from `p`; the package
exports `infer` the way it exports its siblings."""
import numpy as np
import pytest

import jspsr_amd
from jspsr_amd import data as D
from jspsr_amd import infer as I
from tests import batches_ref as B


def test_device_scenes_still_needs_a_ground_truth():
    scenes = B.make_scenes([(40, 40)])
    lists = {k: [s[k] for s in scenes] for k in ("lr_dem", "image", "mask")}
    p = {k: v for k, v in B.PARAMS.items()}
    with pytest.raises(KeyError, match="hr_dem"):
        D.DeviceScenes(hr_dem=None, device="cpu", **lists, **p)
    p.pop("label_range", None)
    S = I.InferenceScenes(device="cpu", **lists, **p)
    assert "hr_dem" not in S.store and isinstance(S, D.DeviceScenes)


def model_and_sample(side=40):
    from jspsr_amd.JSPSR import Model
    model = Model({"lr_dem": 1, "image": 3, "COP30": 1}, num_feature=8)
    s = B.make_scenes([(side, side)])[0]
    return model, {"lr_dem": s["lr_dem"], "image": s["image"]}


def test_upscale_dem_names_a_missing_elevation_range():
    model, sample = model_and_sample()
    p = {"mask_channel": None, "relative": False, "model_name": "JSPSR", "input_data": {"lr_dem": 1, "image": 3}}
    for kw in (None, {}, {"log": True}, {"min": -80}, {"max": 933, "log": True}):
        with pytest.raises(ValueError, match="min and max"):
            I.upscale_dem(model, sample, dict(p, tensor_kwargs=kw))


def test_upscale_dem_checks_input_data_for_a_concatenated_input_only():
    """The reference reads input_data only for the channel count of the concatenated tensor (utils/utils.py:1603-1610)."""
    model, sample = model_and_sample(64)
    p = {"mask_channel": None, "relative": False, "tensor_kwargs": {"min": -80, "max": 933, "log": True}, "model_name": "EDSR"}
    for bad in ({"lr_dem": 1}, {"lr_dem": 1, "image": 1}, {"lr_dem": 1, "image": 3, "mask": 15}):
        with pytest.raises(ValueError, match="input_data"):
            I.upscale_dem(model, sample, dict(p, input_data=bad))


def test_the_package_exports_infer_as_its_siblings():
    assert jspsr_amd.__all__ == ["_lib"]                            # no module is pulled in by `import *`, infer included
    import jspsr_amd.infer as mod                                   # each is imported by name, like data / tiles / summary
    assert mod is I and callable(mod.predict_scenes) and callable(mod.upscale_dem)
    assert np.array_equal(mod.frame_maps(3, 3, 1, 1)[0], [0, 0, 1, 2, 1])


def test_upscale_dem_refuses_rasters_that_are_not_whole_bytes():
    """Image and mask alike: a float image in [0, 1] or a value above 255 is refused, not truncated or wrapped."""
    model, sample = model_and_sample(64)
    p = {"mask_channel": None, "relative": False, "tensor_kwargs": {"min": -80, "max": 933, "log": True}, "model_name": "JSPSR",
         "input_data": {"lr_dem": 1, "image": 3}}
    for bad in (sample["image"].astype(np.float32) / 255, sample["image"].astype(np.int32) + 256):
        with pytest.raises(ValueError, match="image"):
            I.upscale_dem(model, dict(sample, image=bad), p)
    mask = np.full((64, 64, 15), 0.5, dtype=np.float32)
    with pytest.raises(ValueError, match="mask"):
        I.upscale_dem(model, dict(sample, mask=mask), dict(p, input_data={"lr_dem": 1, "image": 3, "mask": 15}))
