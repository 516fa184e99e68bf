"""Training and validation batches made on the device (K9, csrc/batch.hip).

The reference's loader decodes a scene's files, then runs `RandomCrop` -> `RandomFlipRotate90` -> `ToTensor` on the CPU for
every sample and stacks the samples in `DFC30.collate_fn` (data/dfc30.py:193-246,346-364; data/data_utils.py:9-312).
Here decoding stays on the host; everything after it runs on the GPU:

    scenes = DeviceScenes(lr_dem=[...], hr_dem=[...], image=[...], mask=[...], relative=True,
                          elev_min=-80, elev_max=933, elev_log=True, scale_mask=True)
    for batch in RandomCropBatches(scenes, 50, 128, generator=g):
        inputs, gt, base, meta = batch_pair(batch, "JSPSR", input_data)
        loss = criterion(model(*inputs), gt)

`DeviceScenes` uploads the decoded HWC rasters once (the configs' `preload: True`).  `RandomCropBatches` makes the crop and
D4 draws on the host from numpy's random stream, in the reference's order.  Each batch is then ONE launch of
`jspsr_batch_make`, which writes every raster of the batch.  Nothing syncs with the host per step.
"""
from __future__ import annotations

import math
from typing import Iterable, Sequence

import numpy as np
import torch

from . import _lib
from .tiles import get_tile

KINDS = ("lr_dem", "hr_dem", "image", "mask", "canopy", "coord")   # the C ABI's kind indices 0..5
CONCAT_ORDER = ("lr_dem", "image", "mask", "canopy", "coord")      # EDSR's input, utils/utils.py:248-315
GUIDES = ("image", "mask", "canopy")                                # the kinds `guide_resample` takes on finer grids (K26)
_DTYPE = {"lr_dem": np.float32, "hr_dem": np.float32, "image": np.uint8, "mask": np.uint8, "canopy": np.uint8}
LOG, SCALE_MASK, IMAGE_11, LABEL_11, IMAGE_255 = 1, 2, 4, 8, 16   # JSPSR_BATCH_* (include/jspsr_hip.h)
ROW = 8                                                            # int32 words per sample-table row


def d4_code(angle: int, flip_lr: bool, flip_ud: bool) -> int:
    """The kernel's code of np.rot90(., angle), then fliplr, then flipud (data_utils.py:12-30)."""
    return int(angle) * 4 + 2 * bool(flip_lr) + bool(flip_ud)


def _as_hwc(a, kind: str, i: int) -> np.ndarray:
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim != 3 or a.dtype != _DTYPE[kind]:
        raise ValueError(f"{kind}[{i}]: expected an HWC {np.dtype(_DTYPE[kind]).name} array, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def void_pixels(a: np.ndarray, nodata) -> np.ndarray:
    """The voids of an fp32 raster: not finite, or -- unless `nodata` is NaN -- equal to np.float32(nodata)."""
    v = ~np.isfinite(a)
    nd = np.float32(nodata)
    return v if np.isnan(nd) else v | (a == nd)


def _whole(name: str, v) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 0:
        raise ValueError(f"{name}: a whole number of pixels >= 0, got {v!r}")
    return int(v)


class DeviceScenes:
    """Decoded scenes, uploaded once, in the layout `DFC30.__getitem__` holds them: lr_dem / hr_dem fp32 (H,W,1), image
    uint8 (H,W,3), mask uint8 (H,W,C) (the `mask_channel` selection already applied), canopy uint8 (H,W,1); lists of numpy
    arrays or CPU tensors, one entry per scene.  Scenes may differ in size; every kind of a scene has the same H and W.

    Each scene's base elevation is `np.min(lr_dem)` when `relative` (dfc30.py:200), else 0.  The reference asserts its
    ranges per crop (data_utils.py:253-279, 297-299).  Here they are checked once per WHOLE scene at preload: the log domain
    `min - base - elev_min >= 1` and every scaled value in [0, 1].  The scaling is monotone, so a scene that passes cannot
    give a crop that fails.  This is stricter than the reference: a scene whose only bad pixels no crop ever covers is
    refused here.  `elev_min` / `elev_max` are the config's Python numbers (tensor_kwargs min / max).

    Voids (no-data pixels) of the GROUND TRUTH (K19): `hr_nodata=v` marks an hr_dem pixel as a void if it is not finite or
    equals `np.float32(v)` (`void_pixels`' rule; v = NaN: not finite only), and `valid=[per-scene (H,W) uint8 / bool
    planes]` is ANDed in (a water mask, or an `InferenceScenes.void_out == 0`).  Either keyword gives the store the member
    `store["valid"]`: one byte per pixel, 1 = valid, all scenes back to back at the pixel offsets of `scene_table`, padded
    to a multiple of 4 bytes.  hr_dem is uploaded unchanged, voids included; the batches then carry `batch["valid"]`
    ((B,1,k,k) uint8, lined up with `batch["hr_dem"]` under every crop and D4 code, a second launch: jspsr_batch_valid),
    which the masked criterion takes: `criterion(pred, gt, valid=batch["valid"])` -- a masked pixel has no influence whatever
    the rasters hold there.  The hr_dem range checks read the valid pixels only; a scene without a valid hr_dem pixel is a
    ValueError naming it.  With both keywords None nothing changes and "valid" is absent from the store and the batches.
    lr_dem must still be finite: voids in lr_dem AND hr_dem of one store are not built, so `nodata` (the lr_dem voids of
    `infer.InferenceScenes`, filled on the device at construction, K17) still raises NotImplementedError together with
    hr_dem.  Scores over the valid pixels only are `summary.summarise(valid=...)` with `summary.valid_plane` (K18).

    lr_dem at its own resolution (K25, csrc/resample.hip, `resample.resample_rasters`): with `lr_resample="bicubic"` (or
    "bilinear") lr_dem[i] may be smaller than the other rasters of scene i -- a 30 m DEM under 8 m imagery, any ratio >= 1 per
    axis, the extents taken as equal as `F.interpolate(size=)` takes them.  The other rasters fix the scene's shape; a store
    without any needs `lr_shape=(H, W)` (or one pair per scene).  The coarse raster is what is uploaded; base, range checks
    (and void detection) read it; ONE launch at construction then resamples every scene to its shape, clamped to the
    [min, max] of its valid coarse pixels (`lr_clamp`), so that bicubic overshoot cannot leave the range the host checked,
    go below the `relative` base or reach the log of a non-positive number.  `shapes` holds the scenes' (fine) shapes,
    `lr_shapes` the coarse ones; after construction the store is what host-resampled scenes would have given, and batches,
    prepare and every pass downstream are unchanged.  lr_resample=None (the default) keeps requiring equal shapes.

    Imagery at its own resolution (K26, csrc/area.hip, `resample.area_rasters`): with `guide_resample="area"` image[i],
    mask[i] and canopy[i] may each lie on a FINER grid of their own -- 0.5-2 m orthophotos and land cover under an 8 m scene,
    any ratio >= 1 per axis, independent per kind and per scene, the extents taken as equal.  The scene's shape is hr_dem's
    where the store has one, else lr_dem's when `lr_resample` is None, else `lr_shape=` (required then: the guidance rasters
    fix nothing).  The fine rasters are what is uploaded and what the mask and canopy range checks read (a maximum of <= 1 or
    <= 68 survives a mean); ONE launch per kind at construction then brings every scene to its shape: image and canopy by
    the exact area mean rounded half up, the one-hot mask by the majority rule (the class of largest coverage, the lowest
    index among equals, if it covers at least as much as no class does).  `store[kind]` is the result, the fine buffer is
    dropped, `guide_shapes[kind]` keeps the shapes the rasters came in.  A guidance raster smaller than its scene on either
    axis is a ValueError.  Afterwards the store is what host-resampled rasters would have given, bit for bit, and
    `lr_resample`, `nodata`, batches, prepare and every pass downstream work on it unchanged.  guide_resample=None (the
    default) keeps requiring equal shapes.
    """

    def __init__(self, lr_dem: Sequence, hr_dem: Sequence, image=None, mask=None, canopy=None, coord=None, *,
                 relative: bool = False, elev_min: float, elev_max: float, elev_log: bool = False, scale_mask: bool = False,
                 mask_channel: Sequence[int] | None = None, image_range: str | None = None, label_range: str | None = None,
                 normalize: Sequence[str] | None = None, ids: Sequence[str] | None = None, device="cuda", nodata=None,
                 hr_nodata=None, valid=None, lr_resample: str | None = None, lr_shape=None, guide_resample: str | None = None):
        if hr_dem is None:                      # only `infer.InferenceScenes` builds a store without a ground truth
            raise KeyError("hr_dem")
        if nodata is not None:
            raise NotImplementedError("nodata: voids of lr_dem in a store with hr_dem are not built (`infer.InferenceScenes` "
                                      "takes them); the voids of the ground truth are `hr_nodata=` / `valid=`, and "
                                      "`summary.summarise(valid=...)` scores over valid pixels")
        self._setup({"lr_dem": lr_dem, "hr_dem": hr_dem, "image": image, "mask": mask, "canopy": canopy}, coord, relative=relative,
                    elev_min=elev_min, elev_max=elev_max, elev_log=elev_log, scale_mask=scale_mask, mask_channel=mask_channel,
                    image_range=image_range, label_range=label_range, normalize=normalize, ids=ids, device=device,
                    hr_nodata=hr_nodata, valid=valid, lr_resample=lr_resample, lr_shape=lr_shape, guide_resample=guide_resample)

    def _setup(self, raw: dict, coord, *, relative, elev_min, elev_max, elev_log, scale_mask, mask_channel, image_range,
               label_range, normalize, ids, device, base=None, nodata=None, void_margin=0, fill_limit=None, hr_nodata=None,
               valid=None, lr_resample=None, lr_shape=None, guide_resample=None):
        """Checks, layout and upload of a store holding the kinds of `raw` that are not None (`infer.InferenceScenes` is
        the same store without hr_dem).  base: per-scene base elevations instead of `np.min(lr_dem)`.  nodata, void_margin,
        fill_limit: the voids of lr_dem (K17, `infer.InferenceScenes`); nodata=None changes nothing.  hr_nodata, valid: the
        voids of hr_dem (K19, see the class docstring); both None changes nothing.  lr_resample, lr_shape: lr_dem on a
        coarser grid of its own (K25, see the class docstring); lr_resample=None changes nothing.  guide_resample: image,
        mask and canopy on finer grids of their own (K26, see the class docstring); None changes nothing."""
        lr_dem = raw["lr_dem"]
        if guide_resample not in (None, "area"):
            raise ValueError(f"guide_resample must be None or 'area', got {guide_resample!r}")
        guided = guide_resample is not None
        if lr_resample is not None:
            from . import resample                                   # resample imports infer, which imports this module
            resample._mode(lr_resample)
        void_margin = _whole("void_margin", void_margin)
        fill_limit = None if fill_limit is None else _whole("fill_limit", fill_limit)
        if nodata is not None and raw.get("hr_dem") is not None:
            raise NotImplementedError("nodata: voids in a store with hr_dem are not built")
        if coord not in (None, "local"):
            if str(coord).lower() == "global":
                raise NotImplementedError("coord='global' needs the scenes' georeferencing; only 'local' is built")
            raise ValueError(f"coord must be None, 'local' or 'global', got {coord!r}")
        if normalize:
            raise NotImplementedError("Normalize is not built (the reference advises against it, data_utils.py:315)")
        for name, r in (("image_range", image_range), ("label_range", label_range)):
            if r not in (None, "[0, 1]", "[-1, 1]", "[0, 255]"):
                raise ValueError(f"{name} {r!r}")
        if not elev_max > elev_min:
            raise ValueError(f"elev_max {elev_max} <= elev_min {elev_min}")
        self.device = torch.device(device)
        self.relative, self.elev_min, self.elev_max, self.elev_log = relative, elev_min, elev_max, elev_log
        self.scale_mask, self.image_range, self.label_range = scale_mask, image_range, label_range
        self.mask_channel = list(mask_channel) if mask_channel else [*range(15)]      # ToTensor's default (data_utils.py:215)
        n = len(lr_dem)
        if n == 0:
            raise ValueError("no scenes")
        host = {}
        for kind, lst in raw.items():
            if lst is None:
                continue
            if len(lst) != n:
                raise ValueError(f"{kind}: {len(lst)} scenes, lr_dem has {n}")
            host[kind] = [_as_hwc(a, kind, i) for i, a in enumerate(lst)]
        self.kinds = [k for k in KINDS if k in host] + (["coord"] if coord else [])
        self.channels = {k: host[k][0].shape[2] for k in host}
        if coord:
            self.channels["coord"] = 2
        for kind in ("lr_dem", "hr_dem", "canopy"):
            if kind in host and self.channels[kind] != 1:
                raise ValueError(f"{kind} has {self.channels[kind]} channels, not 1")
        self.lr_shapes = [a.shape[:2] for a in host["lr_dem"]]
        self.shapes = self.lr_shapes if lr_resample is None else self._fine_shapes(host, lr_shape, guided)
        if lr_resample is None and lr_shape is not None:
            raise ValueError("lr_shape: only together with lr_resample")
        if guided:
            self.guide_shapes = {k: [tuple(a.shape[:2]) for a in host[k]] for k in GUIDES if k in host}
        for kind, arrs in host.items():
            for i, a in enumerate(arrs):
                if guided and kind in GUIDES and a.shape[2] == self.channels[kind]:
                    if a.shape[0] < self.shapes[i][0] or a.shape[1] < self.shapes[i][1]:
                        raise ValueError(f"{kind}[{i}] is {a.shape[0]} x {a.shape[1]}, its scene {self.shapes[i][0]} x "
                                         f"{self.shapes[i][1]}: upsampling of image / mask / canopy is not built")
                    if max(a.shape[:2]) > 65535:
                        raise ValueError(f"{kind}[{i}] is {a.shape[0]} x {a.shape[1]}: guide_resample takes sides up to 65535")
                    continue
                if a.shape[2] != self.channels[kind] or a.shape[:2] != (self.lr_shapes if kind == "lr_dem" else self.shapes)[i]:
                    raise ValueError(f"{kind}[{i}] {a.shape} does not match lr_dem {host['lr_dem'][i].shape} / "
                                     f"{self.channels[kind]} channels" if lr_resample is None else
                                     f"{kind}[{i}] {a.shape} does not match the scene's {self.shapes[i]} / {self.channels[kind]} channels")
            if self.channels[kind] > 16:
                raise ValueError(f"{kind}: {self.channels[kind]} channels, the kernel takes at most 16")
        if coord and any(h < 2 or w < 2 for h, w in self.shapes):
            raise ValueError("local coordinates need scenes of at least 2 x 2 pixels")
        self.ids = [str(i) for i in range(n)] if ids is None else [str(i) for i in ids]
        voids = None
        if nodata is not None:
            voids = [void_pixels(a, nodata) for a in host["lr_dem"]]
            for i, v in enumerate(voids):
                if v.all():
                    raise ValueError(f"scene {self.ids[i]}: no valid pixel, every lr_dem value is a void")
            self.base = [np.min(a[~v]) if relative else 0 for a, v in zip(host["lr_dem"], voids)]
        else:
            self.base = [np.min(a) if relative else 0 for a in host["lr_dem"]]
        if base is not None:
            if len(base) != n:
                raise ValueError(f"base: {len(base)} values, lr_dem has {n} scenes")
            self.base = list(base)
        planes = None
        if hr_nodata is not None or valid is not None:
            planes = self._valid_planes(host, hr_nodata, valid)
        for i in range(n):
            s = {k: v[i] for k, v in host.items()}
            if voids is not None:
                s["lr_dem"] = s["lr_dem"][~voids[i]]                 # the range checks read the valid pixels only
            if planes is not None:
                s["hr_dem"] = s["hr_dem"][planes[i]]
            self._check_scene(i, s)
        offs = np.zeros(n + 1, dtype=np.int64)
        offs[1:] = np.cumsum([h * w for h, w in self.shapes])
        self.scene_table = torch.tensor([[int(offs[i]), h, w] for i, (h, w) in enumerate(self.shapes)], dtype=torch.int64,
                                        device=self.device)
        # one flat buffer per kind; the store is never modified
        self.store = {k: torch.from_numpy(np.concatenate([a.reshape(-1) for a in v])).to(self.device) for k, v in host.items()
                      if lr_resample is None or k != "lr_dem"}
        if guided:
            self._resample_guides()
        self.flags = ((LOG if elev_log else 0) | (SCALE_MASK if scale_mask else 0) | (IMAGE_11 if image_range == "[-1, 1]" else 0)
                      | (LABEL_11 if label_range == "[-1, 1]" else 0) | (IMAGE_255 if image_range == "[0, 255]" else 0))
        if lr_resample is not None:
            self._resample_lr(host["lr_dem"], voids, nodata, void_margin, fill_limit, lr_resample)
        elif voids is not None:
            self._fill_voids(voids, nodata, void_margin, fill_limit)
        if planes is not None:                   # K19: one byte per pixel at the scenes' pixel offsets, padded to 4 bytes
            flat = np.concatenate([p.reshape(-1) for p in planes]).astype(np.uint8)
            self.store["valid"] = torch.from_numpy(np.concatenate([flat, np.zeros(-flat.size % 4, dtype=np.uint8)])).to(self.device)
            self.hr_nodata = hr_nodata

    hr_nodata = None                             # K19: the no-data value `store["valid"]` was made with, if any

    def _valid_planes(self, host: dict, hr_nodata, valid) -> list:
        """Per-scene (H, W) bool planes of the hr_dem pixels that count: not a void by `hr_nodata`, and set in `valid`."""
        if "hr_dem" not in host:
            raise ValueError("hr_nodata / valid: the store has no hr_dem")
        n = len(host["hr_dem"])
        for i, a in enumerate(host["lr_dem"]):
            if not np.isfinite(a).all():
                raise ValueError(f"scene {self.ids[i]}: lr_dem is not finite; voids in lr_dem and hr_dem of one store are not built")
        if valid is not None and len(valid) != n:
            raise ValueError(f"valid: {len(valid)} planes, hr_dem has {n} scenes")
        planes = []
        for i, a in enumerate(host["hr_dem"]):
            p = np.ones(a.shape[:2], dtype=bool) if hr_nodata is None else ~void_pixels(a[..., 0], hr_nodata)
            if valid is not None:
                u = valid[i].cpu().numpy() if isinstance(valid[i], torch.Tensor) else np.asarray(valid[i])
                if u.dtype not in (np.uint8, np.bool_) or u.shape != a.shape[:2]:
                    raise ValueError(f"valid[{i}]: expected a uint8 or bool plane of {a.shape[:2]}, got {u.dtype} {u.shape}")
                p = p & (u != 0)
            if not p.any():
                raise ValueError(f"scene {self.ids[i]}: no valid pixel, every hr_dem value is a void or masked")
            planes.append(p)
        return planes

    # K17: the members of a store built with `nodata`; None otherwise (and then absent from the instance)
    nodata = void = void_out = void_counts = None
    void_margin, fill_limit = 0, None

    def _fill_voids(self, voids: list, nodata, void_margin: int, fill_limit):
        """The device side of `nodata` (K17, csrc/scene_voids.hip), once, at construction: upload the void plane, replace
        every void of store["lr_dem"] by its nearest valid pixel of the same scene (`infer.nearest_seed`'s rule; farther than
        `fill_limit`: the scene's base) and make the output mask, void or within `void_margin` of one.  A store without a
        single void launches nothing and keeps its bits."""
        from . import infer                                          # infer imports this module
        self.nodata, self.void_margin, self.fill_limit = nodata, void_margin, fill_limit
        self.void_counts = [int(v.sum()) for v in voids]
        plane = np.concatenate([v.reshape(-1) for v in voids]).astype(np.uint8)
        self.void = torch.from_numpy(plane).to(self.device)
        self.void_out = self.void
        if sum(self.void_counts) == 0:
            return
        host_table = infer._host_table(self.shapes)
        self._fill(self.store["lr_dem"], self.void, self.scene_table, host_table, fill_limit)
        if void_margin > 0:
            self.void_out = self._margin(self.void, self.scene_table, host_table, void_margin)

    def _fill(self, dem, void, table, host_table, fill_limit):
        """Every void of the flat buffer `dem` <- its nearest valid pixel of the same scene, or the scene's base."""
        from . import infer
        src = None
        if fill_limit is None or fill_limit > 0:
            src, _ = infer._nearest_seed(void ^ 1, table, host_table, fill_limit or 0)
        base = torch.tensor([float(np.float32(b)) for b in self.base], dtype=torch.float32, device=self.device)
        infer.fill_voids(dem, void, src, table, base)

    @staticmethod
    def _margin(void, table, host_table, void_margin):
        """The output mask: void, or within the Euclidean distance `void_margin` of one."""
        from . import infer
        _, d2 = infer._nearest_seed(void, table, host_table, void_margin)
        return (d2 >= 0).to(torch.uint8)

    lr_clamp = None                              # K25: per-scene (lo, hi) the resampled lr_dem was clamped to, if any
    guide_shapes = None                          # K26: kind -> per-scene (h, w) the guidance rasters came in, if guide_resample

    def _resample_guides(self):
        """The device side of `guide_resample` (K26, csrc/area.hip), once, at construction: the fine rasters of image, mask
        and canopy are what was uploaded; ONE launch per kind brings every scene's raster to the scene's shape -- the exact
        area mean for image and canopy, the majority rule for the one-hot mask -- and the fine buffer is dropped."""
        from . import infer, resample
        for kind, shapes in self.guide_shapes.items():
            self.store[kind], _ = resample.area_rasters(self.store[kind], infer._host_table(shapes), self.channels[kind], self.shapes,
                                                        "majority" if kind == "mask" else "area")

    def _fine_shapes(self, host: dict, lr_shape, guided: bool = False) -> list:
        """The scenes' shapes under `lr_resample`: those of the rasters other than lr_dem, else `lr_shape` -- one (H, W) for
        all scenes or one per scene.  No side of a scene may be shorter than its lr_dem's.  Under `guide_resample` image,
        mask and canopy have grids of their own and fix nothing: hr_dem does, else `lr_shape`."""
        n = len(host["lr_dem"])
        others = [k for k in host if k != "lr_dem" and not (guided and k in GUIDES)]
        if lr_shape is not None:
            given = np.asarray(lr_shape, dtype=np.int64)
            if given.shape not in ((2,), (n, 2)):
                raise ValueError(f"lr_shape: one (H, W) or one per scene, got shape {given.shape}")
            given = [tuple(int(v) for v in (given if given.ndim == 1 else given[i])) for i in range(n)]
        if others:
            fine = [tuple(host[others[0]][i].shape[:2]) for i in range(n)]
            if lr_shape is not None and fine != given:
                raise ValueError(f"lr_shape {given} does not match the shapes of {others[0]}: {fine}")
        elif lr_shape is None:
            raise ValueError("lr_resample: the store has no other raster to take the scenes' shapes from: give lr_shape=(H, W)")
        else:
            fine = given
        for i, ((h, w), (H, W)) in enumerate(zip(self.lr_shapes, fine)):
            if H < h or W < w:
                raise ValueError(f"lr_dem[{i}] is {h} x {w}, its scene {H} x {W}: downsampling needs a prefilter and is not built")
        return fine

    def _resample_lr(self, coarse: list, voids, nodata, void_margin: int, fill_limit, mode: str):
        """The device side of `lr_resample` (K25, csrc/resample.hip), once, at construction: upload lr_dem on its own grid,
        with `nodata` fill its voids there (K17, `fill_limit` in coarse pixels), then ONE launch resamples every scene to its
        shape, clamped to the [min, max] of its valid coarse pixels, and writes the void plane of the fine grid beside it (a
        fine pixel is a void where its centre tap, the coarse pixel at the floor of its coordinate, is); `void_margin` is applied on the fine grid."""
        from . import infer, resample
        host_table = infer._host_table(self.lr_shapes)
        table = torch.from_numpy(host_table).to(self.device)
        lr = torch.from_numpy(np.concatenate([a.reshape(-1) for a in coarse])).to(self.device)
        void = None
        if voids is not None:
            self.nodata, self.void_margin, self.fill_limit = nodata, void_margin, fill_limit
            self.void_counts = [int(v.sum()) for v in voids]                   # counted on lr_dem's own grid
            void = torch.from_numpy(np.concatenate([v.reshape(-1) for v in voids]).astype(np.uint8)).to(self.device)
            if sum(self.void_counts) > 0:
                self._fill(lr, void, table, host_table, fill_limit)
        good = [a if voids is None else a[~voids[i]] for i, a in enumerate(coarse)]
        self.lr_clamp = [(np.float32(g.min()), np.float32(g.max())) for g in good]
        out = resample.resample_rasters(lr, host_table, self.shapes, mode, clamp=self.lr_clamp, void=void)
        self.store["lr_dem"] = out[0]
        if void is not None:
            self.void = self.void_out = out[2]
            if void_margin > 0 and sum(self.void_counts) > 0:
                self.void_out = self._margin(self.void, self.scene_table, infer._host_table(self.shapes), void_margin)

    def void_mask(self, i: int, out: bool = False) -> torch.Tensor:
        """(H, W) bool view on the device of scene i's voids; out=True: of its output mask (void or within `void_margin`
        of one).  Only for a store built with `nodata`."""
        plane = self.void_out if out else self.void
        if plane is None:
            raise ValueError("void_mask: the store was built without nodata")
        if not 0 <= int(i) < len(self):
            raise IndexError(f"scene {i} of {len(self)}")
        h, w = self.shapes[int(i)]
        o = sum(a * b for a, b in self.shapes[:int(i)])
        return plane[o:o + h * w].view(h, w).view(torch.bool)

    def __len__(self):
        return len(self.shapes)

    def scale_dem(self, a: np.ndarray, base) -> np.ndarray:
        """ToTensor.scale_data in numpy, as the reference runs it (data_utils.py:289-312)."""
        data = a.astype(np.float32)
        if base != 0:
            data = data - base
        if self.elev_log:
            assert np.min(data) - self.elev_min >= 1, \
                f"elev_min must smaller than (data - 1) for [0, 1] range: {np.min(data)} {self.elev_min}"
            return np.log(data - self.elev_min) / np.log(self.elev_max - self.elev_min) + 1e-8
        return (data - self.elev_min) / (self.elev_max - self.elev_min)

    def _check_scene(self, i: int, s: dict):
        """The reference's per-crop range asserts, once over the whole scene (see the class docstring)."""
        for kind in ("lr_dem", "hr_dem"):
            if kind not in s:
                continue
            v = self.scale_dem(s[kind], self.base[i])
            if not (v.min() >= 0 and v.max() <= 1):
                raise AssertionError(f"scene {self.ids[i]} {kind}: scaled to [{v.min()}, {v.max()}], not within [0, 1]")
        if "mask" in s:
            m = s["mask"].astype(np.float32)
            if self.scale_mask:
                m = m * (np.arange(m.shape[2], dtype=np.float32) + 1) / np.float32(len(self.mask_channel) + 1)
            if not (m.min() >= 0 and m.max() <= 1):
                raise AssertionError(f"scene {self.ids[i]} mask: values within [{m.min()}, {m.max()}], not [0, 1]")
        if "canopy" in s and s["canopy"].max() > 68:
            raise AssertionError(f"scene {self.ids[i]} canopy: {s['canopy'].max()} > 68")

    def make(self, table: torch.Tensor, k: int, outs: dict):
        """One launch: table (B, 8) int32 sample rows on the device; outs kind -> (tensor (B, cpitch, k, k), coff)."""
        lib = _lib.load()
        P = ctypes_arrays(self, outs)
        B = table.shape[0]
        _lib.check(lib.jspsr_batch_make(P[0], P[1], P[2], P[3], P[4], P[5], self.scene_table.data_ptr(), len(self), table.data_ptr(),
                                        B, k, self.flags, float(self.elev_min), float(self.elev_max),
                                        len(self.mask_channel) + 1, torch.cuda.current_stream(self.device).cuda_stream),
                   "jspsr_batch_make")

    def make_valid(self, table: torch.Tensor, k: int) -> torch.Tensor:
        """The batch's validity plane, (B, 1, k, k) uint8, from the same sample rows (K19, one launch of jspsr_batch_valid);
        only for a store built with `hr_nodata` or `valid`."""
        plane = self.store["valid"]
        B = table.shape[0]
        out = torch.empty((B, 1, k, k), dtype=torch.uint8, device=self.device)
        _lib.check(_lib.load().jspsr_batch_valid(plane.data_ptr(), plane.numel(), out.data_ptr(), self.scene_table.data_ptr(),
                                                 len(self), table.data_ptr(), B, k,
                                                 torch.cuda.current_stream(self.device).cuda_stream), "jspsr_batch_valid")
        return out


def ctypes_arrays(scenes: DeviceScenes, outs: dict):
    """The six-entry host arrays of jspsr_batch_make (include/jspsr_hip.h)."""
    import ctypes
    src = (ctypes.c_void_p * 6)()
    nbytes = (ctypes.c_longlong * 6)()
    out = (ctypes.c_void_p * 6)()
    ch, coff, pitch = (ctypes.c_int * 6)(), (ctypes.c_int * 6)(), (ctypes.c_int * 6)()
    for i, kind in enumerate(KINDS):
        if kind not in outs:
            continue
        t, c0 = outs[kind]
        if kind in scenes.store:
            st = scenes.store[kind]
            src[i], nbytes[i] = st.data_ptr(), st.numel() * st.element_size()
        out[i] = t.data_ptr()
        ch[i], coff[i], pitch[i] = scenes.channels[kind], c0, t.shape[1]
    return src, nbytes, out, ch, coff, pitch


class ShuffleOrder:
    """The index order of `DataLoader(dataset, shuffle=True, generator=g, num_workers=0)`: each epoch the loader's iterator
    first draws its base seed from `g` (or torch's global generator), then RandomSampler draws the permutation."""

    def __init__(self, n: int, generator: torch.Generator | None = None):
        self.n, self.generator = n, generator

    def __len__(self):
        return self.n

    def __iter__(self):
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)
        return iter(torch.utils.data.RandomSampler(range(self.n), generator=self.generator))


class _Batches:
    """Shared part of the two batch iterables: output allocation, the launch and the yielded dict."""

    def __init__(self, scenes: DeviceScenes, batch_size: int, patch_size: int, concat: bool):
        if batch_size <= 0 or patch_size <= 0:
            raise ValueError("batch_size and patch_size must be positive")
        self.scenes, self.batch_size, self.k, self.concat = scenes, batch_size, patch_size, concat

    def _upload(self, rows: np.ndarray) -> torch.Tensor:
        """One stream-ordered copy of a whole table from a pinned buffer that is never written again (a new one per call:
        the caching host allocator keeps a freed block until the copies from it are done)."""
        host = torch.empty(rows.shape, dtype=torch.int32, pin_memory=True)
        host.numpy()[...] = rows
        return host.to(self.scenes.device, non_blocking=True)

    def _launch(self, table: torch.Tensor, side: int, meta: list) -> dict:
        S, B = self.scenes, table.shape[0]
        kw = dict(dtype=torch.float32, device=S.device)
        batch, outs = {}, {}
        if self.concat:
            C = sum(S.channels[k] for k in CONCAT_ORDER if k in S.channels)
            images = torch.empty((B, C, side, side), **kw)
            c0 = 0
            for kind in CONCAT_ORDER:
                if kind in S.channels:
                    outs[kind] = (images, c0)
                    batch[kind] = images[:, c0:c0 + S.channels[kind]]
                    c0 += S.channels[kind]
            outs["hr_dem"] = (torch.empty((B, 1, side, side), **kw), 0)
            batch["hr_dem"] = outs["hr_dem"][0]
            batch["images"] = images
        else:
            for kind in S.kinds:
                outs[kind] = (torch.empty((B, S.channels[kind], side, side), **kw), 0)
                batch[kind] = outs[kind][0]
        S.make(table, side, outs)
        if "valid" in S.store:                               # K19: a second launch, only for a store that has the plane
            batch["valid"] = S.make_valid(table, side)
        batch["base"] = table[:, 4].view(torch.float32)      # (B,) fp32 view of the rows' base elevations, on the device
        batch["meta"] = meta
        return batch

    def _meta(self, s: int, bbox, aug) -> dict:
        S = self.scenes
        return {"id": S.ids[s], "base": S.base[s], "bbox": bbox,
                "augmentation": {"rot90": aug[0], "flip_lr": aug[1], "flip_ud": aug[2]}}

    def _side(self, s: int) -> int:
        h, w = self.scenes.shapes[s]
        if self.k > h or self.k > w or self.k == h == w:          # no crop (data_utils.py:53-54, 108-109)
            if h != w:
                raise ValueError(f"scene {self.scenes.ids[s]} ({h} x {w}) is not cropped and not square: it cannot be stacked")
            return h
        return self.k

    def _run(self, table: torch.Tensor, sides: list, metas: list):
        B = self.batch_size
        for lo in range(0, len(sides), B):
            hi = min(lo + B, len(sides))
            side = set(sides[lo:hi])
            if len(side) != 1:
                raise ValueError(f"samples of sides {sorted(side)} in one batch cannot be stacked")
            yield self._launch(table[lo:hi], side.pop(), metas[lo:hi])


class RandomCropBatches(_Batches):
    """The training batches: `DataLoader(DFC30(transform=RandomCrop -> RandomFlipRotate90 -> ToTensor), batch_size,
    shuffle=True, drop_last=True, collate_fn=DFC30.collate_fn)` with the samples made on the device.

    sampler: any iterable of scene indices (a DistributedSampler works); default `ShuffleOrder(len(scenes), generator)`.
    rng: the numpy RandomState the draws come from; default numpy's global one, as the reference draws.  Per sample, in the
    reference's order: randint(0, h-k-1) for the row, randint(0, w-k-1) for the column (h, w of the scene; no draw when the
    crop is skipped), then with `augment` random_sample() < 0.5 and, if so, choice([1,2,3]), choice([True, False]) for
    flip_lr and for flip_ud.  All draws of an epoch are made when its iteration starts (the reference makes them as each
    batch is fetched: the stream is the same unless the caller draws from the same RandomState in between).
    Each yielded dict holds the present rasters as (B, C, k, k) fp32 device tensors, `base` (B,) on the device and `meta`
    as collate_fn gives it.  concat=True writes [lr_dem | image | mask | canopy | coord] into one tensor `images` (EDSR's
    input) and gives the kinds as its channel slices.  A store built with `hr_nodata` / `valid` adds `valid`, the
    (B, 1, k, k) uint8 plane of the hr_dem pixels that count (K19).
    """

    def __init__(self, scenes: DeviceScenes, batch_size: int, patch_size: int, augment: bool = True, rng=None,
                 sampler: Iterable[int] | None = None, drop_last: bool = True, generator: torch.Generator | None = None,
                 concat: bool = False):
        super().__init__(scenes, batch_size, patch_size, concat)
        self.augment, self.rng, self.drop_last = augment, rng, drop_last
        self.sampler = ShuffleOrder(len(scenes), generator) if sampler is None else sampler

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def draw(self, indices: Sequence[int]):
        """Host draws for these samples: (rows (n, 8) int32, sides, metas)."""
        r = self.rng if self.rng is not None else np.random.mtrand._rand
        rows = np.zeros((len(indices), ROW), dtype=np.int32)
        sides, metas = [], []
        k = self.k
        for j, s in enumerate(indices):
            s = int(s)
            h, w = self.scenes.shapes[s]
            side = self._side(s)
            if side == k and not (k == h == w):
                y0, x0 = int(r.randint(0, h - k - 1)), int(r.randint(0, w - k - 1))
                bbox = (y0, x0, y0 + k, x0 + k)
            else:
                y0 = x0 = 0
                bbox = (0, 0, h, w)
            aug = (0, False, False)
            if self.augment and r.random_sample() < 0.5:
                aug = (int(r.choice([1, 2, 3])), bool(r.choice([True, False])), bool(r.choice([True, False])))
            rows[j, :4] = (s, y0, x0, d4_code(*aug))
            rows[j, 4] = np.float32(self.scenes.base[s]).view(np.int32)
            sides.append(side)
            metas.append(self._meta(s, bbox, aug))
        return rows, sides, metas

    def __iter__(self):
        idx = [int(i) for i in self.sampler]
        if self.drop_last:
            idx = idx[:len(idx) // self.batch_size * self.batch_size]
        if not idx:
            return
        rows, sides, metas = self.draw(idx)
        yield from self._run(self._upload(rows), sides, metas)


class TileCropBatches(_Batches):
    """The validation batches (crop_mode: tile): sample i is tile i % n of scene i // n, row-major over the cover
    `tiles.get_tile(W, k, n)` (TileCrop, data_utils.py:87-168), no augmentation, in order, the last batch kept.  meta's
    bbox is TileCrop's (x0, y0, x0 + k, y0 + k)."""

    def __init__(self, scenes: DeviceScenes, batch_size: int, patch_size: int, patches_per_image: int, concat: bool = False):
        super().__init__(scenes, batch_size, patch_size, concat)
        self.n = patches_per_image
        rows, self.sides, self.metas = [], [], []
        for s in range(len(scenes)):
            h, w = scenes.shapes[s]
            side = self._side(s)
            cover = [(0, 0)] * self.n
            if side == self.k and not (self.k == h == w):
                stride, n = get_tile(w, self.k, self.n)
                if n != self.n:
                    raise ValueError(f"scene {scenes.ids[s]}: a {n}-tile cover, not {self.n}")
                n_x = math.isqrt(n)
                cover = [(stride * (t // n_x), stride * (t % n_x)) for t in range(n)]
            for y0, x0 in cover:
                bbox = (x0, y0, x0 + self.k, y0 + self.k) if side == self.k and not (self.k == h == w) else (0, 0, h, w)
                rows.append([s, y0, x0, 0, np.float32(scenes.base[s]).view(np.int32), 0, 0, 0])
                self.sides.append(side)
                self.metas.append(self._meta(s, bbox, (0, False, False)))
        self.rows = np.array(rows, dtype=np.int32).reshape(-1, ROW)
        self._table = None

    def __len__(self):
        return math.ceil(len(self.sides) / self.batch_size)

    def __iter__(self):
        if self._table is None:
            self._table = self._upload(self.rows)
        yield from self._run(self._table, self.sides, self.metas)


def batch_pair(batch: dict, model_name: str, input_data: dict):
    """(inputs, hr_dem, base_elev, meta) as get_batch_pair returns them (utils/utils.py:152-315), from a device batch.
    JSPSR / LRRU: inputs = [lr_dem, image, mask, canopy, coord], the kinds input_data names.  Any other model (EDSR): inputs
    = [images], the concatenated tensor the kernel wrote (a batch made with concat=True)."""
    name = (model_name or "").lower()
    if name in {"jspsr", "lrru"}:
        inputs = [batch["lr_dem"]] + [batch[k] for k in ("image", "mask", "canopy", "coord") if k in input_data]
    elif name == "completionformer":
        raise NotImplementedError("the completionformer split input is not built")
    else:
        if "images" not in batch:
            raise ValueError(f"{model_name} takes one concatenated input: make the batches with concat=True")
        want = [k for k in CONCAT_ORDER[1:] if k in input_data]
        have = [k for k in CONCAT_ORDER[1:] if k in batch]
        if want != have:
            raise ValueError(f"input_data asks for {want}, the batch holds {have}")
        inputs = [batch["images"]]
    return inputs, batch["hr_dem"], batch["base"], batch["meta"]
