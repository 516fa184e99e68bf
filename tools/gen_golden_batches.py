"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/g11_batches.npz: training samples made by the reference's own
transforms (data/data_utils.py: RandomCrop -> RandomFlipRotate90 -> ToTensor, the order get_transformations builds for a
DFC dataset with augment on, utils/common_config.py:112-161; and one TileCrop -> ToTensor pass), on the synthetic scenes
of tests/batches_ref.py, with DFC30.__getitem__'s sample dict and meta (data/dfc30.py:193-246).

The reference is imported as oracle/gen_golden.py:import_reference does, with placeholder modules for what this image
lacks.  torchvision.transforms.ToTensor is absent: the stand-in below restates torchvision's to_tensor for uint8 HWC
arrays only (CHW, float, div(255)).  affine.Affine is absent: a stand-in carries TileCrop's profile bookkeeping, which is
not stored.

Run where the reference tree is available (never on the GPU box):

    python tools/gen_golden_batches.py

The fixture stores the seeds and the scenes' checksum, so the tests regenerate the scenes and fail on a mismatch.
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402
from tests import batches_ref as R  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g11_batches.npz")


class _ToTensor:
    """torchvision.transforms.ToTensor on a uint8 HWC array: CHW, float32, divided by 255."""

    def __call__(self, a):
        assert a.dtype == np.uint8 and a.ndim == 3
        return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class _Affine:
    def __init__(self, *c):
        self.c = c

    def __getitem__(self, i):
        return self.c[i]

    def __mul__(self, xy):
        a, b, c, d, e, f = self.c
        return (a * xy[0] + b * xy[1] + c, d * xy[0] + e * xy[1] + f)


def import_data_utils():
    G.import_reference()
    tv = sys.modules["torchvision"]
    tr = types.ModuleType("torchvision.transforms")
    tr.ToTensor = _ToTensor
    tv.transforms = tr
    sys.modules["torchvision.transforms"] = tr
    aff = types.ModuleType("affine")
    aff.Affine = _Affine
    sys.modules["affine"] = aff
    import data.data_utils as du
    return du


def get_item(scenes, i, relative):
    """DFC30.__getitem__'s sample dict (key order and meta) for scene i of the synthetic set."""
    s = scenes[i]
    h, w = s["lr_dem"].shape[:2]
    sample = {k: s[k] for k in R.KIND_ORDER if k in s}
    sample["meta"] = {"id": str(i), "subset": "synthetic", "shape": (h, w, sum(a.shape[2] for a in sample.values())),
                      "augmentation": {"rot90": 0, "flip_lr": False, "flip_ud": False}, "bbox": (0, 0, h, w),
                      "base": np.min(s["lr_dem"]) if relative else 0,
                      "profile": {"transform": _Affine(3.0, 0.0, 1000.0, 0.0, -3.0, 2000.0), "width": w, "height": h}}
    return sample


def main():
    du = import_data_utils()
    p = R.PARAMS
    scenes = R.make_scenes()
    to_tensor = du.ToTensor(None, p["mask_channel"], p["relative"], min=p["elev_min"], max=p["elev_max"], log=p["elev_log"],
                            scale_mask=p["scale_mask"])
    store = {"seed": np.int64(R.SEED), "draw_seed": np.int64(R.DRAW_SEED), "k": np.int64(R.K), "shapes": np.array(R.SHAPES),
             "order": np.array(R.ORDER), "tile_scenes": np.array(R.TILE_SCENES), "tile_n": np.int64(R.TILE_N),
             "scenes_checksum": np.array(R.scenes_checksum(scenes))}

    def record(prefix, chain, order):
        res = []
        for j, i in enumerate(order):
            s = get_item(scenes, i, p["relative"])
            for t in chain:
                s = t(s)
            for kind in ("lr_dem", "hr_dem", "image", "mask", "canopy"):
                store[f"{prefix}{j}_{kind}"] = s[kind].numpy()
            m = s["meta"]
            a = m["augmentation"]
            store[f"{prefix}{j}_bbox"] = np.array(m["bbox"], dtype=np.int64)
            store[f"{prefix}{j}_aug"] = np.array([a["rot90"], a["flip_lr"], a["flip_ud"]], dtype=np.int64)
            store[f"{prefix}{j}_base"] = np.float32(m["base"])
            res.append(s)
        return res

    np.random.seed(R.DRAW_SEED)
    got = record("r", [du.RandomCrop(R.K), du.RandomFlipRotate90(), to_tensor], R.ORDER)
    # the restatement must agree with the reference before anything is stored
    ref = R.random_pass(scenes, p, R.K, R.ORDER, np.random.RandomState(R.DRAW_SEED))
    for s, (out, base, bbox, aug) in zip(got, ref):
        assert tuple(s["meta"]["bbox"]) == bbox and tuple(s["meta"]["augmentation"].values()) == aug
        for kind, v in out.items():
            assert np.array_equal(s[kind].numpy(), v), kind
    tile = du.TileCrop(R.K, n_tile=R.TILE_N)
    got = record("t", [tile, to_tensor], [i for i in R.TILE_SCENES for _ in range(R.TILE_N)])
    ref = R.tile_pass(scenes, p, R.K, R.TILE_N, R.TILE_SCENES)
    for s, (out, base, bbox, aug) in zip(got, ref):
        assert tuple(s["meta"]["bbox"]) == bbox
        for kind, v in out.items():
            assert np.array_equal(s[kind].numpy(), v), kind
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
