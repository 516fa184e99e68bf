"""Whole-scene inference on the device (K13, csrc/scene_prepare.hip, scene.hip): raw rasters in, metres out.

The reference's `upscale_dem` (utils/utils.py:1556-1654) pads a decoded scene to a power of two with a mirrored border
(`cal_pad` / `add_padding`, :1501-1553), runs `ToTensor` (data/data_utils.py:217-312) on every raster, calls the model and
removes the border again.  Here each side of the forward is ONE launch, for a batch of equally sized scenes:

    scenes = InferenceScenes(lr_dem=[...], image=[...], mask=[...], relative=True, elev_min=-80, elev_max=933,
                             elev_log=True, scale_mask=True)
    result = predict_scenes(model, scenes, batch_size=8, pad="pow2")          # no host synchronisation
    dems = result.rasters()                                                   # {scene id: (H, W) fp32 metres}

`prepare` gathers the raw HWC bytes of the store through two index maps (`frame_maps`) and applies ToTensor's per-kind
arithmetic -- K9's, bit for bit (csrc/totensor.h).  The maps carry `add_padding`'s mirror border index for index (its
bottom strip sits one row above a true mirror), the extension of the frame to a multiple of the model's `size_multiple`,
and nothing else: all policy is host code.  `finish` reads the window back and, for metres, applies clamp ->
`metrics.descale_data` -> `+ base`, the bits of `summary.compose_scene` on a single uncropped tile.  `upscale_dem` keeps
the reference's own contract on top of the two.

Self-ensemble (K14, csrc/scene_prepare.hip, scene_tta.hip): `predict_scenes(..., tta="d4")` averages the predictions over the four quarter
turns and their mirror images.  `prepare_d4` transforms every raster of a sample on the device BEFORE the padding (the
mirror border is not symmetric), one launch per rot90 parity; `finish_mean` carries up to eight predictions back, averages
them in fp32 in a fixed order and converts to metres, one launch.

Tiled inference (K15, csrc/scene_prepare.hip, scene_tiles.hip): `predict_scenes(..., tile=512, overlap=64, trim=16)` covers every scene that
is larger than the tile with equal windows (`cover.plan_cover`), gathers them straight from the store (`prepare_windows`,
windows of different scenes share a batch), and merges the predictions with the cover's ramp weights in metres
(`merge_windows`, one launch per group of equally shaped scenes).  Activation memory then follows batch_size x tile^2, not
the scene.  This is the reference's validation protocol -- per-tile channel-gate statistics, zero padding at tile edges,
linear ramps over the overlaps -- continued to any scene; it is not an exact decomposition of the monolithic forward
(`tiling.py` is).

Tiled self-ensemble (K16, csrc/scene_prepare.hip): `predict_scenes(..., tile=512, window_tta="d4")` keeps the upright cover
and runs every WINDOW in each orientation: `prepare_windows_d4` gathers and transforms in one launch per rot90 parity,
`mean_windows` (K14's finish_mean, the tile as its scene) carries the predictions back and averages them in fp32, and
`merge_windows` feathers the mean tiles in metres.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Sequence

import numpy as np
import torch

from . import _lib
from . import tiles as T
from .cover import Cover, plan_cover  # noqa: F401  (part of this module's surface)
from .data import CONCAT_ORDER, DeviceScenes, ctypes_arrays

Frame = namedtuple("Frame", "Hp Wp top left H W")     # the padded frame and the scene's window in it

_CACHE_LIMIT = 256                                    # entries of a cache of uploads; a full cache is emptied
_MAPS = {}                                            # (H, W, pad, multiple, device) -> _Uploaded((rows, cols)), Frame


def frame_maps(H: int, W: int, pad: int = 0, multiple: int = 1):
    """-> (rows, cols, top, left): int32 numpy maps with frame[Y][X] = scene[rows[Y]][cols[X]], and the scene's corner.

    With n = pad the frame is (H + 2n + eh) x (W + 2n + ew), eh = -(H + 2n) mod multiple, ew likewise: `add_padding`'s
    border (utils/utils.py:1501-1520) and, past it, its bottom / right rule continued until the side is a multiple.
      rows: Y < n -> n-1-Y;  Y < H+n -> Y-n;  else 2H+n-2-Y    (the reference's bottom strip, one row above a mirror)
      cols: X < n -> n-1-X;  X < W+n -> X-n;  else 2W+n-1-X
    ValueError unless n <= H, n + eh <= H - 1 and n + ew <= W: the conditions under which every entry is inside the scene."""
    H, W, n, m = int(H), int(W), int(pad), int(multiple)
    if H < 1 or W < 1 or n < 0 or m < 1:
        raise ValueError(f"frame_maps: H {H}, W {W}, pad {n}, multiple {m}")
    eh, ew = (-(H + 2 * n)) % m, (-(W + 2 * n)) % m
    if not (n <= H and n + eh <= H - 1 and n + ew <= W):
        raise ValueError(f"frame_maps: a {H} x {W} scene cannot fill a border of {n} and an extension of {eh} rows, {ew} "
                         f"columns (needs pad <= H, pad + rows <= H - 1, pad + columns <= W)")
    Y = np.arange(H + 2 * n + eh, dtype=np.int64)
    X = np.arange(W + 2 * n + ew, dtype=np.int64)
    rows = np.where(Y < n, n - 1 - Y, np.where(Y < H + n, Y - n, 2 * H + n - 2 - Y)).astype(np.int32)
    cols = np.where(X < n, n - 1 - X, np.where(X < W + n, X - n, 2 * W + n - 1 - X)).astype(np.int32)
    return rows, cols, n, n


class _Uploaded:
    """Small int32 arrays copied to the device once and kept: one stream-ordered copy each from a pinned buffer that is
    never written again (as data._Batches._upload), on the stream that is current at the first use.  A later use may be on
    another stream, which nothing orders behind that copy, so the copies are followed by an event: `on_current_stream`
    makes the current stream wait for it on the device (no host synchronisation) until the copies are seen to be
    complete, and tells the allocator about a stream other than the first, so that the memory of an evicted entry is not
    handed out again under a kernel that still reads it."""

    def __init__(self, hosts, device):
        self.device = device
        self.stream = torch.cuda.current_stream(device)
        self.tensors = []
        for host in hosts:
            pinned = torch.empty(host.shape, dtype=torch.int32, pin_memory=True)
            pinned.numpy()[...] = host
            self.tensors.append(pinned.to(device, non_blocking=True))
        self.event = torch.cuda.Event()
        self.event.record(self.stream)

    def on_current_stream(self):
        stream = torch.cuda.current_stream(self.device)
        if self.event is not None:
            if self.event.query():
                self.event = None
            elif stream != self.stream:
                stream.wait_event(self.event)
        if stream != self.stream:
            for t in self.tensors:
                t.record_stream(stream)
        return self.tensors


def _cached(cache, key, device, build):
    """The entry `key` of a cache of uploads: on its first use build() -> (int32 host arrays, anything to keep beside
    them) is uploaded (`_Uploaded`), a full cache being emptied first.  -> (the device tensors, ordered for the current
    stream; what was kept)."""
    if key not in cache:
        hosts, kept = build()
        if len(cache) >= _CACHE_LIMIT:
            cache.clear()
        cache[key] = (_Uploaded(hosts, torch.device(device)), kept)
    uploaded, kept = cache[key]
    return uploaded.on_current_stream(), kept


def _store_table(scenes, key, build):
    """`_cached` for the one-array tables kept with a store (`scenes._infer_tables`) -> (device table, what was kept)."""
    tensors, kept = _cached(scenes.__dict__.setdefault("_infer_tables", {}), key, scenes.device, build)
    return tensors[0], kept


def _device_maps(H, W, pad, multiple, device):
    """-> (rows, cols, frame): the device copies of `frame_maps`, cached per geometry and device, ordered for the current
    stream."""
    def build():
        rows, cols, top, left = frame_maps(H, W, pad, multiple)
        return (rows, cols), Frame(len(rows), len(cols), top, left, H, W)
    (rows, cols), frame = _cached(_MAPS, (H, W, pad, multiple, str(device)), device, build)
    return rows, cols, frame


class InferenceScenes(DeviceScenes):
    """`data.DeviceScenes` without a ground truth: decoded scenes, uploaded once, in the same flat HWC layout with the same
    members (`store`, `scene_table`, `base`, `flags`, `channels`, `shapes`, `ids`) and the same whole-scene range checks.
    base: per-scene base elevations to use instead of `np.min(lr_dem)` (upscale_dem's `meta["base"]`).

    Voids (K17, csrc/scene_voids.hip).  nodata=None: no scene may hold one (today's checks, nothing else happens).
    Otherwise an lr_dem pixel is a void when it is not finite, or -- unless nodata is NaN -- equals np.float32(nodata).  The
    base (`np.min` when `relative`) and the range checks then read the valid pixels only; a scene without one is a
    ValueError that names it.  The void plane is uploaded (`void`: flat uint8 in the store's pixel layout; `void_counts` per
    scene; `void_mask(i)`), and once, at construction, every void of store["lr_dem"] is replaced on the device by the value of
    its nearest valid pixel of the same scene (`nearest_seed`'s rule) -- farther than `fill_limit` pixels from valid data:
    by the scene's base; fill_limit=0: every void.  After that the store is read-only and finite: prepare, the ensembles and
    the tiled passes read it unchanged.  `void_out` (`void_mask(i, out=True)`): void, or within the Euclidean distance
    `void_margin` of one (0: `void` itself, the same tensor); `predict_scenes(mask_voids=True)` writes np.float32(nodata)
    there.  Such results are scored over the valid pixels only by `summary.summarise(valid=...)` (K18).  Voids in image, mask
    or canopy and voids together with hr_dem are not built.

    lr_dem at its own resolution (K25, csrc/resample.hip; `data.DeviceScenes` has the whole account).
    lr_resample="bicubic" | "bilinear": lr_dem[i] may be coarser than the other rasters of scene i, which fix the scene's
    shape (no other raster: lr_shape=(H, W), or one pair per scene); it is uploaded as it is and resampled on the device at
    construction, clamped to the [min, max] of its valid pixels.  `shapes` are the scenes' shapes, `lr_shapes` those of
    lr_dem.  With `nodata` the voids are found and filled on lr_dem's own grid (`fill_limit` and `void_counts` in its
    pixels), `void` is written on the scene's grid -- a pixel is a void where its centre tap (the lr_dem pixel at the floor of its
    coordinate) is -- and
    `void_margin` is applied there.  After construction the store is what host-resampled scenes would have given.

    Imagery at its own resolution (K26, csrc/area.hip; `data.DeviceScenes` has the whole account).  guide_resample="area":
    image[i], mask[i] and canopy[i] may each be finer than scene i, any ratio >= 1 per axis; the scene's shape is lr_dem's,
    or `lr_shape=` together with `lr_resample`.  They are uploaded as they are and brought to the scene's grid on the device
    at construction, one launch per kind: the exact area mean for image and canopy, the majority rule for the mask.
    `guide_shapes[kind]` keeps the shapes they came in."""

    def __init__(self, lr_dem: Sequence, image=None, mask=None, canopy=None, coord=None, *, relative: bool = False,
                 elev_min: float, elev_max: float, elev_log: bool = False, scale_mask: bool = False,
                 mask_channel: Sequence[int] | None = None, image_range: str | None = None, ids: Sequence[str] | None = None,
                 device="cuda", base: Sequence | None = None, nodata=None, void_margin: int = 0, fill_limit: int | None = None,
                 lr_resample: str | None = None, lr_shape=None, guide_resample: str | None = None):
        self._setup({"lr_dem": lr_dem, "hr_dem": None, "image": image, "mask": mask, "canopy": canopy}, coord, relative=relative,
                    elev_min=elev_min, elev_max=elev_max, elev_log=elev_log, scale_mask=scale_mask, mask_channel=mask_channel,
                    image_range=image_range, label_range=None, normalize=None, ids=ids, device=device, base=base,
                    nodata=nodata, void_margin=void_margin, fill_limit=fill_limit, lr_resample=lr_resample, lr_shape=lr_shape,
                    guide_resample=guide_resample)


def _input_kinds(scenes):
    return [k for k in CONCAT_ORDER if k in scenes.channels]


def _rows_of(scenes, indices) -> np.ndarray:
    """The sample table of jspsr_scene_prepare / _finish: (B, 2) int32 {scene, base as fp32 bits}."""
    rows = np.zeros((len(indices), 2), dtype=np.int32)
    for j, s in enumerate(indices):
        if not 0 <= int(s) < len(scenes):
            raise IndexError(f"scene {s} of {len(scenes)}")
        rows[j] = (int(s), np.float32(scenes.base[int(s)]).view(np.int32))
    return rows


def _table(scenes, indices) -> torch.Tensor:
    """The device copy of `_rows_of`, kept with the store per index list and ordered for the current stream: a repeated call
    uploads nothing."""
    key = tuple(int(s) for s in indices)
    return _store_table(scenes, key, lambda: ((_rows_of(scenes, key),), None))[0]


def _one_shape(scenes, indices):
    if len(indices) == 0:
        raise ValueError("no scenes named")
    shapes = {tuple(scenes.shapes[int(s)]) for s in indices}
    if len(shapes) != 1:
        raise ValueError(f"scenes of shapes {sorted(shapes)} cannot share a frame")
    return shapes.pop()


def _inputs(scenes, B, h, w, concat):
    """The fp32 (B, C, h, w) input tensors of a forward, one per kind in `_input_kinds`' order -- concat: one tensor
    [lr_dem | image | ...] --, and outs(lo, hi): kind -> (the samples lo:hi of its tensor, its first channel there), as the
    prepare calls take them."""
    kinds = _input_kinds(scenes)
    C = [scenes.channels[k] for k in kinds]
    kw = dict(dtype=torch.float32, device=scenes.device)
    inputs = [torch.empty((B, sum(C), h, w), **kw)] if concat else [torch.empty((B, c, h, w), **kw) for c in C]

    def outs(lo=0, hi=B):
        return {k: (inputs[0 if concat else j][lo:hi], sum(C[:j]) if concat else 0) for j, k in enumerate(kinds)}
    return inputs, outs


def _launch(entry, scenes, table, outs, codes, *geometry):
    """jspsr_scene_prepare*: the arguments the four entries share, around the host codes (the D4 entries; a ctypes int
    array or a sequence), the sample count and `geometry` -- the maps and the frame's sides, or the tile's sides."""
    import ctypes
    count = (table.shape[0],)
    if codes is not None:
        if not isinstance(codes, ctypes.Array):
            codes = (ctypes.c_int * len(codes))(*[int(c) for c in codes])
        if len(codes) != table.shape[0]:
            raise ValueError(f"{entry[len('jspsr_scene_'):]}: {len(codes)} codes for {table.shape[0]} samples")
        count = (codes, table.shape[0])
    _lib.check(getattr(_lib.load(), entry)(*ctypes_arrays(scenes, outs), scenes.scene_table.data_ptr(), len(scenes), table.data_ptr(),
                                           *count, *geometry, scenes.flags, float(scenes.elev_min), float(scenes.elev_max),
                                           len(scenes.mask_channel) + 1, torch.cuda.current_stream(scenes.device).cuda_stream),
               entry)


def _prepare(scenes, table, H, W, pad, multiple, concat):
    rows, cols, frame = _device_maps(H, W, int(pad), int(multiple), scenes.device)
    inputs, outs = _inputs(scenes, table.shape[0], frame.Hp, frame.Wp, concat)
    launch_prepare(scenes, table, rows, cols, frame.Hp, frame.Wp, outs())
    return inputs, frame


def launch_prepare(scenes, table, rows, cols, Hp, Wp, outs: dict):
    """The raw call: table (B, 2) int32, rows (Hp,) and cols (Wp,) int32 on the device; outs kind -> (tensor of
    (B, cpitch, Hp, Wp) fp32, first channel), as `DeviceScenes.make` takes them."""
    _launch("jspsr_scene_prepare", scenes, table, outs, None, rows.data_ptr(), cols.data_ptr(), Hp, Wp)


def prepare(scenes, indices: Sequence[int], pad: int = 0, multiple: int = 8, concat: bool = False):
    """One launch: the scenes `indices` of the store (all of one shape) -> (inputs, frame).  inputs: the model's fp32
    (B, C, Hp, Wp) tensors in `data.batch_pair`'s order [lr_dem, image, mask, canopy, coord], the kinds the store holds;
    concat=True: one tensor [lr_dem | image | ...] (EDSR's input).  frame: `Frame(Hp, Wp, top, left, H, W)`."""
    H, W = _one_shape(scenes, indices)
    return _prepare(scenes, _table(scenes, indices), H, W, pad, multiple, concat)


def _finish(pred, table, scenes, frame, metres, out):
    B = table.shape[0]
    if pred.dim() == 3:
        pred = pred[:, None]
    if tuple(pred.shape) != (B, 1, frame.Hp, frame.Wp):
        raise ValueError(f"finish: predictions {tuple(pred.shape)}, expected {(B, 1, frame.Hp, frame.Wp)}")
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"finish: fp32 or bf16 predictions, got {pred.dtype}")
    if pred.device != scenes.device:
        raise ValueError(f"finish: predictions on {pred.device}, the scenes on {scenes.device}")
    pred = pred.detach().contiguous()
    _lib.check(_lib.load().jspsr_scene_finish(int(pred.dtype == torch.bfloat16), pred.data_ptr(), out.data_ptr(), table.data_ptr(),
                                              B, frame.Hp, frame.Wp, frame.top, frame.left, frame.H, frame.W, int(bool(metres)),
                                              int(bool(scenes.elev_log)), float(scenes.elev_min), float(scenes.elev_max),
                                              torch.cuda.current_stream(scenes.device).cuda_stream), "jspsr_scene_finish")
    return out


def finish(pred: torch.Tensor, scenes, indices: Sequence[int], frame: Frame, metres: bool = True) -> torch.Tensor:
    """One launch: predictions (B, 1, Hp, Wp) in the network's range (fp32 or bf16) -> (B, H, W) fp32, the scenes' window
    of the frame.  metres=True: clamp to [0, 1] -> `metrics.descale_data` -> + the scene's base elevation (NaN stays NaN);
    metres=False: the window as it is (what upscale_dem returns)."""
    _one_shape(scenes, indices)
    out = torch.empty((len(indices), frame.H, frame.W), dtype=torch.float32, device=scenes.device)
    return _finish(pred, _table(scenes, indices), scenes, frame, metres, out)


# ---- K14 (csrc/scene_prepare.hip, scene_tta.hip): the self-ensemble over the flips and quarter turns -----------------------
def _element(e):
    """-> (rot90, flip_lr, flip_ud) from a triple or from K9's code rot90 * 4 + flip_lr * 2 + flip_ud."""
    if isinstance(e, (int, np.integer)) and not isinstance(e, (bool, np.bool_)):
        if not 0 <= int(e) < 16:
            raise ValueError(f"D4 code {e} outside 0..15")
        return int(e) >> 2, bool(int(e) & 2), bool(int(e) & 1)
    try:
        r, lr, ud = e
    except (TypeError, ValueError):
        raise ValueError(f"a D4 element is (rot90, flip_lr, flip_ud) or a code 0..15, got {e!r}") from None
    if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, np.integer)) or not 0 <= int(r) < 4:
        raise ValueError(f"D4 element {e!r}: rot90 must be 0..3")
    for f in (lr, ud):
        if not isinstance(f, (bool, np.bool_)) and f not in (0, 1):
            raise ValueError(f"D4 element {e!r}: the flips must be booleans")
    return int(r), bool(lr), bool(ud)


def d4_code(element) -> int:
    r, lr, ud = _element(element)
    return r * 4 + lr * 2 + ud


def d4_canonical(element):
    """The same element with flip_ud clear: flipud = fliplr after a half turn, so the 16 codes are 8 elements."""
    r, lr, ud = _element(element)
    return ((r + 2) % 4, not lr, False) if ud else (r, lr, False)


def d4_elements(spec="d4") -> list:
    """"d4": the eight elements (r, lr, False), r = 0..3, lr = False, True, in that order; None: the identity alone; a
    sequence of triples (rot90, flip_lr, flip_ud) or codes: those, as triples, in the order given.  ValueError on a bad
    value, on an empty sequence and on two entries that denote the same element."""
    if spec is None:
        return [(0, False, False)]
    if isinstance(spec, str):
        if spec.lower() != "d4":
            raise ValueError(f"tta: 'd4', None or a sequence of elements, got {spec!r}")
        return [(r, lr, False) for r in range(4) for lr in (False, True)]
    out, seen = [], {}
    for e in spec:
        t = _element(e)
        c = d4_canonical(t)
        if c in seen:
            raise ValueError(f"tta: {seen[c]} and {t} are the same element")
        seen[c] = t
        out.append(t)
    if not out:
        raise ValueError("tta: no elements")
    return out


def d4_apply(a, element, axes=(0, 1)):
    """flipud?(fliplr?(rot90(a, rot90))) over `axes` of a numpy array: the reference's RandomFlipRotate90 order
    (data/data_utils.py:26-28)."""
    r, lr, ud = _element(element)
    a = np.rot90(a, r, axes)
    a = np.flip(a, axes[1]) if lr else a
    return np.flip(a, axes[0]) if ud else a


def d4_invert(a, element, axes=(0, 1)):
    """The inverse of `d4_apply`: d4_invert(d4_apply(a, e), e) is a."""
    r, lr, ud = _element(element)
    a = np.flip(a, axes[0]) if ud else a
    a = np.flip(a, axes[1]) if lr else a
    return np.rot90(a, -r, axes)


def _frame_d4(scenes, H, W, parity, pad, multiple, element):
    """The frame of the transformed shape: (W, H) for an odd rot90; pad after the transform."""
    h, w = (W, H) if parity else (H, W)
    n = T.cal_pad(h, w) if pad == "pow2" else int(pad)
    try:
        return _device_maps(h, w, n, int(multiple), scenes.device)
    except ValueError as err:
        raise ValueError(f"frame_maps: element {element} turns the {H} x {W} scene into {h} x {w}: {err}") from None


def _table_d4(scenes, indices, codes):
    """(device table (len(codes) * B, 3) int32 {scene, base as fp32 bits, code}, element-major; the host codes), kept with
    the store per (index list, codes) as `_table` keeps its tables."""
    key = ("d4", tuple(int(s) for s in indices), tuple(int(c) for c in codes))
    return _store_table(scenes, key, lambda: _coded(_rows_of(scenes, key[1]), key[2]))


def _coded(rows, codes):
    """A sample table once per code, element-major, the code as one more column -> ((the table,), the ctypes copy of that
    column): what `_store_table` uploads and keeps for a D4 entry."""
    import ctypes
    rows = np.concatenate([np.concatenate([rows, np.full((len(rows), 1), c, dtype=np.int32)], axis=1) for c in codes])
    return (rows,), (ctypes.c_int * len(rows))(*rows[:, -1].tolist())


def launch_prepare_d4(scenes, table, codes, rows, cols, Hp, Wp, outs: dict):
    """The raw call: table (B, 3) int32 on the device, codes its third column on the host (a ctypes int array or a
    sequence); the rest as `launch_prepare`, the maps those of the transformed shape."""
    _launch("jspsr_scene_prepare_d4", scenes, table, outs, codes, rows.data_ptr(), cols.data_ptr(), Hp, Wp)


def _parity_order(elements):
    return [e for e in elements if e[0] % 2 == 0] + [e for e in elements if e[0] % 2 == 1]


def _run(scenes, nb, order, h, w, concat, launch):
    """One forward's inputs for the samples (element, one of nb scenes or windows), element-major, `order` being
    `_parity_order`'s and of one output shape h x w: launch(parity, codes, outs) per rot90 parity present, the even one
    first, into batch slices of the same tensors."""
    inputs, outs = _inputs(scenes, len(order) * nb, h, w, concat)
    at = 0
    for p in (0, 1):
        codes = [d4_code(e) for e in order if e[0] % 2 == p]
        if codes:
            launch(p, codes, outs(at, at + len(codes) * nb))
            at += len(codes) * nb
    return inputs


def _prepare_run(scenes, idx, elements, H, W, pad, multiple, concat):
    """The samples (element, scene), element-major, of one forward: `elements` must share a frame shape (one rot90 parity,
    or a square scene).  One launch per parity into batch slices of the same tensors, the even elements first.
    -> (inputs, {parity: Frame}, the elements in batch order)."""
    order = _parity_order(elements)
    maps = {p: _frame_d4(scenes, H, W, p, pad, multiple, next(e for e in order if e[0] % 2 == p)) for p in {e[0] % 2 for e in order}}
    shapes = {(f.Hp, f.Wp) for _, _, f in maps.values()}
    if len(shapes) != 1:
        raise ValueError(f"elements {order} of a {H} x {W} scene have frames {sorted(shapes)}: one rot90 parity per forward")
    Hp, Wp = shapes.pop()

    def launch(p, codes, outs):
        table, host = _table_d4(scenes, idx, codes)
        launch_prepare_d4(scenes, table, host, maps[p][0], maps[p][1], Hp, Wp, outs)
    return _run(scenes, len(idx), order, Hp, Wp, concat, launch), {p: f for p, (_, _, f) in maps.items()}, order


def prepare_d4(scenes, indices: Sequence[int], elements="d4", pad=0, multiple: int = 8, concat: bool = False) -> dict:
    """One launch per rot90 parity: the D4 elements `elements` (`d4_elements`) of the scenes `indices` (all of one shape),
    transformed, THEN padded and brought to ToTensor's range -> {parity: (inputs, frame, order)}.  inputs as `prepare`
    gives them, the samples element-major: order[j] = (position in `indices`, element) of sample j.  frame: the frame of
    the transformed shape, (W, H) for parity 1, with the same border and multiple.  The bits of `prepare` on a store of
    the host-transformed rasters; coord holds the local coordinates of the source pixel."""
    H, W = _one_shape(scenes, indices)
    elements = d4_elements(elements)
    idx = [int(s) for s in indices]
    out = {}
    for p in (0, 1):
        es = [e for e in elements if e[0] % 2 == p]
        if es:
            inputs, frames, order = _prepare_run(scenes, idx, es, H, W, pad, multiple, concat)
            out[p] = (inputs, frames[p], [(j, e) for e in order for j in range(len(idx))])
    return out


def _mean(who, preds, frames, elements, table, out, H, W, metres, elev_log, elev_min, elev_max, device, elsewhere):
    """jspsr_scene_finish_mean: preds[k] (B, 1, Hp_k, Wp_k) on `device`, the prediction of element elements[k] with its H x W
    scene (or tile) at frames[k]; the messages start with `who` and name the other device as `elsewhere`."""
    B = table.shape[0]
    variants = (_lib.TtaVariant * max(len(preds), 1))()
    keep = []
    for k, (pred, frame, e) in enumerate(zip(preds, frames, elements)):
        if pred.dim() == 3:
            pred = pred[:, None]
        if tuple(pred.shape) != (B, 1, frame.Hp, frame.Wp):
            raise ValueError(f"{who}: predictions {tuple(pred.shape)} of element {e}, expected {(B, 1, frame.Hp, frame.Wp)}")
        if pred.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{who}: fp32 or bf16 predictions, got {pred.dtype}")
        if pred.device != device:
            raise ValueError(f"{who}: predictions on {pred.device}{elsewhere}")
        pred = pred.detach().contiguous()
        keep.append(pred)
        if k < len(variants):
            variants[k] = _lib.TtaVariant(pred.data_ptr(), int(pred.dtype == torch.bfloat16), d4_code(e), frame.Hp, frame.Wp,
                                          frame.top, frame.left, frame.H, frame.W)
    _lib.check(_lib.load().jspsr_scene_finish_mean(variants, len(preds), out.data_ptr(), table.data_ptr(), B, H, W,
                                                   int(bool(metres)), int(bool(elev_log)), float(elev_min), float(elev_max),
                                                   torch.cuda.current_stream(device).cuda_stream), "jspsr_scene_finish_mean")
    return out


def _finish_mean(preds, table, scenes, frames, elements, H, W, metres, out):
    return _mean("finish_mean", preds, frames, elements, table, out, H, W, metres, scenes.elev_log, scenes.elev_min, scenes.elev_max,
                 scenes.device, f", the scenes on {scenes.device}")


def finish_mean(preds: Sequence[torch.Tensor], scenes, indices: Sequence[int], frames, elements, metres: bool = True) -> torch.Tensor:
    """One launch: preds[k] (B, 1, Hp_k, Wp_k), fp32 or bf16, the model's output for element elements[k] of the scenes
    `indices` -> (B, H, W) fp32: every window carried back by the inverse of its element, (((y'_0 + y'_1) + y'_2) + ...) / K
    in fp32 in the order given, then `finish`'s metres (or nothing).  frames: {parity: Frame} as `prepare_d4` returns them,
    or one Frame per prediction.  One element alone, the identity: the bits of `finish`.  A NaN anywhere makes the pixel NaN."""
    H, W = _one_shape(scenes, indices)
    elements = [_element(e) for e in elements]
    if len(preds) != len(elements):
        raise ValueError(f"finish_mean: {len(preds)} predictions for {len(elements)} elements")
    if isinstance(frames, dict):
        frames = [frames[e[0] % 2] for e in elements]
    if len(frames) != len(elements):
        raise ValueError(f"finish_mean: {len(frames)} frames for {len(elements)} elements")
    out = torch.empty((len(indices), H, W), dtype=torch.float32, device=scenes.device)
    return _finish_mean(list(preds), _table(scenes, indices), scenes, frames, elements, H, W, metres, out)


def _ensemble_chunks(elements, square, batch_size):
    """How an ensemble rides the batch dimension -> (nb, runs): chunks of nb scenes (or windows), and per chunk one forward
    per run of elements, nb * len(run) <= batch_size samples where that leaves room for one.  The elements of a square shape
    share one output shape; a rectangle's rot90 parities have one each, the even one first."""
    even, odd = [e for e in elements if e[0] % 2 == 0], [e for e in elements if e[0] % 2 == 1]
    sets = [even + odd] if square else [s for s in (even, odd) if s]
    nb = max(1, batch_size // max(len(s) for s in sets))
    per = max(1, batch_size // nb)                                         # elements per forward
    return nb, [s[e0:e0 + per] for s in sets for e0 in range(0, len(s), per)]


def _predict_tta(model, scenes, indices, elements, groups, offsets, buffer, batch_size, pad, multiple, concat, take, metres):
    """predict_scenes' pass with a self-ensemble: per group of equally shaped scenes, chunks of scenes whose variants ride
    the batch dimension, at most `batch_size` samples per forward; a square scene's elements share one frame shape, a
    rectangular scene's rot90 parities have one each."""
    for (h, w), members in groups.items():
        nb, runs = _ensemble_chunks(elements, h == w, batch_size)
        for lo in range(0, len(members), nb):
            idx = [indices[pos] for pos in members[lo:lo + nb]]
            preds, frames = {}, {}
            for run in runs:
                inputs, fr, order = _prepare_run(scenes, idx, run, h, w, pad, multiple, concat)
                pred = model(*[inputs[i] for i in take])
                if pred.shape[0] != len(order) * len(idx):
                    raise ValueError(f"predict_scenes: {len(order) * len(idx)} samples in, {pred.shape[0]} predictions out")
                pred = pred.detach().contiguous()
                for j, e in enumerate(order):
                    preds[e], frames[e] = pred[j * len(idx):(j + 1) * len(idx)], fr[e[0] % 2]
            o = offsets[members[lo]]
            _finish_mean([preds[e] for e in elements], _table(scenes, idx), scenes, [frames[e] for e in elements], elements, h, w,
                         metres, buffer[o:o + len(idx) * h * w])


# ---- K15 (csrc/scene_prepare.hip, scene_tiles.hip): scenes of any size through tiles of one size -------------------------
_COVERS = {}                                          # (Cover.key, device) -> _Uploaded((oy, ox, lo_y, lo_x, wy bits, wx bits))


def _tile_sides(tile):
    if isinstance(tile, (int, np.integer)) and not isinstance(tile, (bool, np.bool_)):
        kh = kw = int(tile)
    else:
        try:
            kh, kw = (int(t) for t in tile)
        except (TypeError, ValueError):
            raise ValueError(f"tile: an int or (kh, kw), got {tile!r}") from None
    if kh < 1 or kw < 1:
        raise ValueError(f"tile: positive sides, got {(kh, kw)}")
    return kh, kw


def _device_cover(cover: Cover, device):
    """-> (oy, ox, lo_y, lo_x, wy, wx) on the device (the weights as their int32 bit patterns), cached per cover and device
    and ordered for the current stream, as `_device_maps`."""
    def hosts():
        return (cover.oy, cover.ox, cover.lo_y, cover.lo_x, np.ascontiguousarray(cover.wy, np.float32).view(np.int32),
                np.ascontiguousarray(cover.wx, np.float32).view(np.int32)), None
    return _cached(_COVERS, (cover.key, str(device)), device, hosts)[0]


def _window_rows(scenes, windows) -> np.ndarray:
    """The sample table of jspsr_scene_prepare_windows: (B, 4) int32 {scene, base as fp32 bits, y0, x0}."""
    rows = np.zeros((len(windows), 4), dtype=np.int32)
    for j, (s, y0, x0) in enumerate(windows):
        if not 0 <= int(s) < len(scenes):
            raise IndexError(f"scene {s} of {len(scenes)}")
        rows[j] = (int(s), np.float32(scenes.base[int(s)]).view(np.int32), int(y0), int(x0))
    return rows


def _window_table(scenes, windows) -> torch.Tensor:
    """The device copy of `_window_rows`, kept with the store per window list as `_table` keeps its tables."""
    key = ("windows", tuple((int(s), int(y), int(x)) for s, y, x in windows))
    return _store_table(scenes, key, lambda: ((_window_rows(scenes, key[1]),), None))[0]


def launch_prepare_windows(scenes, table, kh, kw, outs: dict):
    """The raw call: table (B, 4) int32 on the device; outs kind -> (tensor of (B, cpitch, kh, kw) fp32, first channel)."""
    _launch("jspsr_scene_prepare_windows", scenes, table, outs, None, kh, kw)


def _prepare_windows(scenes, table, kh, kw, concat):
    inputs, outs = _inputs(scenes, table.shape[0], kh, kw, concat)
    launch_prepare_windows(scenes, table, kh, kw, outs())
    return inputs


def prepare_windows(scenes, windows: Sequence, tile, concat: bool = False):
    """One launch: the windows (scene, y0, x0) of the store, each `tile` = k or (kh, kw) pixels, of any scenes and shapes ->
    the model's fp32 (B, C, kh, kw) inputs in `prepare`'s order (concat=True: one tensor).  The bits of `prepare(scenes,
    [scene], 0, 1)` at [y0:y0 + kh, x0:x0 + kw] -- the base and the local coordinates are the whole scene's; a window
    pixel outside its scene is NaN."""
    kh, kw = _tile_sides(tile)
    if len(windows) == 0:
        raise ValueError("no windows named")
    return _prepare_windows(scenes, _window_table(scenes, windows), kh, kw, concat)


def _merge_windows(tiles, table, scenes, cover, metres, out):
    S = table.shape[0]
    if tiles.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"merge_windows: fp32 or bf16 predictions, got {tiles.dtype}")
    if tiles.device != scenes.device:
        raise ValueError(f"merge_windows: predictions on {tiles.device}, the scenes on {scenes.device}")
    if tiles.numel() != S * cover.n * cover.kh * cover.kw or tuple(tiles.shape[-2:]) != (cover.kh, cover.kw):
        raise ValueError(f"merge_windows: predictions {tuple(tiles.shape)}, expected {S} x {cover.n} tiles of {cover.kh} x {cover.kw}")
    tiles = tiles.detach().contiguous()
    oy, ox, lo_y, lo_x, wy, wx = _device_cover(cover, scenes.device)
    _lib.check(_lib.load().jspsr_scene_merge_windows(int(tiles.dtype == torch.bfloat16), tiles.data_ptr(), wy.data_ptr(), wx.data_ptr(),
                                                     lo_y.data_ptr(), lo_x.data_ptr(), oy.data_ptr(), ox.data_ptr(), table.data_ptr(),
                                                     out.data_ptr(), S, cover.n_y, cover.n_x, cover.kh, cover.kw, cover.H, cover.W,
                                                     int(bool(metres)), int(bool(scenes.elev_log)), float(scenes.elev_min),
                                                     float(scenes.elev_max), torch.cuda.current_stream(scenes.device).cuda_stream),
               "jspsr_scene_merge_windows")
    return out


def merge_windows(pred_tiles: torch.Tensor, scenes, indices: Sequence[int], cover: Cover, metres: bool = True) -> torch.Tensor:
    """One launch: the predictions (S * n, 1, kh, kw) -- or (S, n, kh, kw) -- of the cover's n tiles, row-major, of the scenes
    `indices` (all of the cover's shape), fp32 or bf16 -> (S, H, W) fp32.  Every tile goes to metres first as `finish`
    does (clamp, de-scale, + base; metres=False: as it is), then acc += (m * wx) * wy over the tiles whose weights at the
    pixel are not zero, row-major.  A tile is not read where its weight is zero."""
    if _one_shape(scenes, indices) != (cover.H, cover.W):
        raise ValueError(f"merge_windows: scenes of {tuple(scenes.shapes[int(indices[0])])}, a cover of {(cover.H, cover.W)}")
    out = torch.empty((len(indices), cover.H, cover.W), dtype=torch.float32, device=scenes.device)
    return _merge_windows(pred_tiles, _table(scenes, indices), scenes, cover, metres, out)


def _tile_plan(scenes, indices, tiled, groups, covers):
    """-> (kh, kw, slot, windows, slots): the tile; position -> first tile of the scene in a tile buffer laid out group by
    group; the windows (scene, y0, x0) of the scenes `tiled` in scene order, row-major; and each window's tile in the
    buffer."""
    kh, kw = next((c.kh, c.kw) for c in covers.values())
    slot, at = {}, 0
    for shape, members in groups.items():
        for pos in members:
            slot[pos] = at
            at += covers[shape].n
    windows, slots = [], []
    for pos in tiled:
        cover = covers[tuple(scenes.shapes[indices[pos]])]
        windows += [(indices[pos], y0, x0) for y0, x0 in cover.windows()]
        slots += range(slot[pos], slot[pos] + cover.n)
    return kh, kw, slot, windows, slots


def _to_slots(tiles, slots, src):
    """tiles[slots[j]] = src[j], one copy per run of consecutive slots: the windows of one scene."""
    j = 0
    while j < len(slots):
        e = j + 1
        while e < len(slots) and slots[e] == slots[e - 1] + 1:
            e += 1
        tiles[slots[j]:slots[j] + e - j].copy_(src[j:e])
        j = e


def _merge_groups(tiles, slot, scenes, indices, groups, covers, offsets, buffer, metres):
    """One merge launch per shape group, from the tile buffer into the result."""
    for shape, members in groups.items():
        idx = [indices[pos] for pos in members]
        h, w = shape
        o, t0 = offsets[members[0]], slot[members[0]]
        _merge_windows(tiles[t0:t0 + len(idx) * covers[shape].n], _table(scenes, idx), scenes, covers[shape], metres,
                       buffer[o:o + len(idx) * h * w])


def _predict_tiled(model, scenes, indices, tiled, groups, covers, offsets, buffer, batch_size, concat, take, metres):
    """predict_scenes' pass over the scenes larger than the tile (`tiled`: their positions in `indices`, ascending; `covers`:
    shape -> Cover, all of one tile).  The windows are listed in scene order, row-major, and cut into forwards of
    `batch_size`; the predictions land in one tile buffer laid out group by group, so that one merge launch per shape group
    writes the result."""
    kh, kw, slot, windows, slots = _tile_plan(scenes, indices, tiled, groups, covers)
    table = _window_table(scenes, windows)
    tiles = None
    for lo in range(0, len(windows), batch_size):
        B = min(batch_size, len(windows) - lo)
        inputs = _prepare_windows(scenes, table[lo:lo + B], kh, kw, concat)
        pred = model(*[inputs[i] for i in take])
        if pred.dim() == 3:
            pred = pred[:, None]
        if tuple(pred.shape) != (B, 1, kh, kw):
            raise ValueError(f"predict_scenes: {B} windows of {kh} x {kw} in, predictions {tuple(pred.shape)} out")
        if tiles is None:
            tiles = torch.empty((len(windows), 1, kh, kw), dtype=pred.dtype, device=scenes.device)
        _to_slots(tiles, slots[lo:lo + B], pred)
    _merge_groups(tiles, slot, scenes, indices, groups, covers, offsets, buffer, metres)


# ---- K16 (csrc/scene_prepare.hip): the self-ensemble per window of a tiled scene -------------------------------------------
def _window_table_d4(scenes, windows, codes):
    """(device table (len(codes) * B, 5) int32 {scene, base as fp32 bits, y0, x0, code}, element-major; the host codes), kept
    with the store per (window list, codes) as `_window_table` keeps its tables."""
    key = ("windows_d4", tuple((int(s), int(y), int(x)) for s, y, x in windows), tuple(int(c) for c in codes))
    return _store_table(scenes, key, lambda: _coded(_window_rows(scenes, key[1]), key[2]))


def launch_prepare_windows_d4(scenes, table, codes, kh, kw, outs: dict):
    """The raw call: table (B, 5) int32 on the device, codes its fifth column on the host (a ctypes int array or a sequence),
    all of one rot90 parity; outs kind -> (tensor of (B, cpitch, kh, kw) fp32 -- (B, cpitch, kw, kh) for an odd rot90 --,
    first channel)."""
    _launch("jspsr_scene_prepare_windows_d4", scenes, table, outs, codes, kh, kw)


def _prepare_windows_run(scenes, windows, elements, kh, kw, concat):
    """The samples (element, window), element-major, of one forward: `elements` must share an output shape (one rot90 parity,
    or a square tile).  One launch per parity into batch slices of the same tensors, the even elements first.
    -> (inputs, the elements in batch order)."""
    order = _parity_order(elements)
    shapes = {(kw, kh) if e[0] % 2 else (kh, kw) for e in order}
    if len(shapes) != 1:
        raise ValueError(f"elements {order} of a {kh} x {kw} window have shapes {sorted(shapes)}: one rot90 parity per forward")
    oh, ow = shapes.pop()

    def launch(p, codes, outs):
        table, host = _window_table_d4(scenes, windows, codes)
        launch_prepare_windows_d4(scenes, table, host, kh, kw, outs)
    return _run(scenes, len(windows), order, oh, ow, concat, launch), order


def prepare_windows_d4(scenes, windows: Sequence, tile, elements="d4", concat: bool = False) -> dict:
    """One launch per rot90 parity: the D4 elements `elements` (`d4_elements`) of the windows (scene, y0, x0) of the store,
    each `tile` = k or (kh, kw) pixels, of any scenes and shapes -> {parity: (inputs, order)}.  inputs as `prepare_windows`
    gives them -- (B, C, kh, kw) for parity 0, (B, C, kw, kh) for parity 1 --, the samples element-major: order[j] = (position
    in `windows`, element) of sample j.  The bits of `prepare_windows` moved by flipud?(fliplr?(rot90(window, rot90))): the
    base and the local coordinates are those of the source pixel in its whole scene, a source pixel outside its scene is
    NaN."""
    kh, kw = _tile_sides(tile)
    if len(windows) == 0:
        raise ValueError("no windows named")
    elements = d4_elements(elements)
    windows = [(int(s), int(y), int(x)) for s, y, x in windows]
    out = {}
    for p in (0, 1):
        es = [e for e in elements if e[0] % 2 == p]
        if es:
            inputs, order = _prepare_windows_run(scenes, windows, es, kh, kw, concat)
            out[p] = (inputs, [(j, e) for e in order for j in range(len(windows))])
    return out


def _mean_windows(preds, elements, kh, kw, table, out):
    """jspsr_scene_finish_mean with the tile as its scene: preds[k] (N, 1, kh, kw) -- (N, 1, kw, kh) for an odd rot90 -- of
    element elements[k]; table a device (N, 2) int32 table (read, not used: metres = 0); out (N, 1, kh, kw) fp32."""
    frames = [Frame(kw, kh, 0, 0, kw, kh) if e[0] % 2 else Frame(kh, kw, 0, 0, kh, kw) for e in elements]
    return _mean("mean_windows", preds, frames, elements, table, out, kh, kw, 0, 0, 0.0, 1.0, out.device, f" and on {out.device}")


def mean_windows(preds: Sequence[torch.Tensor], elements, tile) -> torch.Tensor:
    """One launch: preds[k] (N, 1, kh, kw) -- (N, 1, kw, kh) for an odd rot90 --, fp32 or bf16, the model's output for element
    elements[k] of N windows of `tile` = k or (kh, kw) -> (N, 1, kh, kw) fp32 in the network's range: every tile carried back
    by the inverse of its element, (((y'_0 + y'_1) + y'_2) + ...) / K in fp32 in the order given (`finish_mean` with the tile
    as its scene and metres=False).  One element alone, the identity: the input widened to fp32.  `merge_windows` takes the
    result."""
    kh, kw = _tile_sides(tile)
    elements = [_element(e) for e in elements]
    preds = list(preds)
    if len(preds) != len(elements):
        raise ValueError(f"mean_windows: {len(preds)} predictions for {len(elements)} elements")
    if not preds:
        raise ValueError("mean_windows: no predictions")
    N, device = preds[0].shape[0], preds[0].device
    table = torch.zeros((N, 2), dtype=torch.int32, device=device)
    out = torch.empty((N, 1, kh, kw), dtype=torch.float32, device=device)
    return _mean_windows(preds, elements, kh, kw, table, out)


def _predict_tiled_tta(model, scenes, indices, tiled, groups, covers, offsets, buffer, batch_size, concat, take, metres, elements):
    """`_predict_tiled` with a self-ensemble per window: the windows, listed as there, go in chunks of nb windows whose
    variants ride the batch dimension, at most `batch_size` samples per forward (`_predict_tta`'s rule, the tile in the place
    of the scene: a square tile's elements share one shape, a rectangular tile's rot90 parities have one each).  Per chunk
    one finish_mean launch writes the fp32 mean tiles into the tile buffer; then `_predict_tiled`'s merge."""
    kh, kw, slot, windows, slots = _tile_plan(scenes, indices, tiled, groups, covers)
    nb, runs = _ensemble_chunks(elements, kh == kw, batch_size)
    tiles = torch.empty((len(windows), 1, kh, kw), dtype=torch.float32, device=scenes.device)
    for lo in range(0, len(windows), nb):
        chunk = windows[lo:lo + nb]
        B = len(chunk)
        preds = {}
        for run in runs:
            inputs, order = _prepare_windows_run(scenes, chunk, run, kh, kw, concat)
            pred = model(*[inputs[i] for i in take])
            if pred.dim() == 3:
                pred = pred[:, None]
            if tuple(pred.shape) != (len(order) * B, 1) + tuple(inputs[0].shape[2:]):
                raise ValueError(f"predict_scenes: {len(order) * B} windows of {tuple(inputs[0].shape[2:])} in, predictions "
                                 f"{tuple(pred.shape)} out")
            pred = pred.detach().contiguous()
            for j, e in enumerate(order):
                preds[e] = pred[j * B:(j + 1) * B]
        table = _table(scenes, [w[0] for w in chunk])
        one_run = all(slots[lo + j] == slots[lo] + j for j in range(B))    # the chunk's tiles are neighbours: no copy
        out = tiles[slots[lo]:slots[lo] + B] if one_run else torch.empty((B, 1, kh, kw), dtype=torch.float32, device=scenes.device)
        _mean_windows([preds[e] for e in elements], elements, kh, kw, table, out)
        if not one_run:
            _to_slots(tiles, slots[lo:lo + B], out)
    _merge_groups(tiles, slot, scenes, indices, groups, covers, offsets, buffer, metres)


# ---- K17 (csrc/scene_voids.hip): voids -- the nearest-seed transform, the fill and the output mask ------------------------------
MAX_SIDE = 32767                                      # scene sides of the transform: d2 < 2^31


def _host_table(shapes_or_table) -> np.ndarray:
    """(n, 3) int64 {pixel offset, H, W} on the host from a list of (H, W) shapes (scenes back to back) or from such a
    table, a numpy array or a tensor (a device tensor is copied back: a synchronisation)."""
    a = shapes_or_table
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.int64)
    if a.ndim != 2 or a.shape[1] not in (2, 3) or a.shape[0] == 0:
        raise ValueError(f"nearest_seed: a list of (H, W) shapes or an (n, 3) table {{offset, H, W}}, got shape {a.shape}")
    if a.shape[1] == 3:
        return np.ascontiguousarray(a)
    table = np.zeros((len(a), 3), dtype=np.int64)
    table[:, 1:] = a
    table[1:, 0] = np.cumsum(a[:, 0] * a[:, 1])[:-1]
    return table


def _nearest_seed(seed, table, host_table, limit: int):
    """The raw call: seed flat uint8 on the device, table (n, 3) int64 on the device and its host copy, limit >= 1 or 0 for
    none -> (src, d2) int32.  The workspace (2 B per pixel) is freed on return; the allocator keeps it until the stream
    has passed the launches."""
    if seed.dtype != torch.uint8 or seed.dim() != 1 or not seed.is_contiguous() or not seed.is_cuda:
        raise ValueError(f"nearest_seed: a flat contiguous uint8 plane on the device, got {seed.dtype} {tuple(seed.shape)} on {seed.device}")
    n = seed.numel()
    lib = _lib.load()
    host_table = np.ascontiguousarray(host_table, dtype=np.int64)
    src = torch.empty(n, dtype=torch.int32, device=seed.device)
    d2 = torch.empty(n, dtype=torch.int32, device=seed.device)
    work = torch.empty(max(1, lib.jspsr_scene_nearest_seed_workspace_bytes(n)), dtype=torch.uint8, device=seed.device)
    _lib.check(lib.jspsr_scene_nearest_seed(seed.data_ptr(), n, table.data_ptr(), host_table.ctypes.data, len(host_table), int(limit),
                                            src.data_ptr(), d2.data_ptr(), work.data_ptr(),
                                            torch.cuda.current_stream(seed.device).cuda_stream), "jspsr_scene_nearest_seed")
    return src, d2


def nearest_seed(seed: torch.Tensor, shapes_or_scene_table, limit: int | None = None):
    """Three kernels, one call: for every pixel of a flat uint8 device plane `seed` (non-zero = seed) that holds the scenes
    `shapes_or_scene_table` -- a list of (H, W), back to back, or an (n, 3) int64 table {pixel offset, H, W} such as a
    store's `scene_table` -- its nearest seed of the SAME scene -> (src, d2), flat int32 on the device.

    The rule: of all seeds of the scene the one that minimises (dy^2 + dx^2, |dx|, dx, dy) lexicographically, d = seed -
    query.  src = y_s * W + x_s inside the scene, d2 the squared distance; a seed has src = itself, d2 = 0.  Both are -1 where
    the scene has no seed, or none within `limit` pixels (d2 > limit^2; None: no limit; 0: only the seeds themselves find
    one).  Exact and integer: every run gives the same bits.  Sides are at most 32767."""
    host = _host_table(shapes_or_scene_table)
    if limit is not None and (isinstance(limit, (bool, np.bool_)) or not isinstance(limit, (int, np.integer)) or int(limit) < 0):
        raise ValueError(f"nearest_seed: limit is None or a whole number >= 0, got {limit!r}")
    if isinstance(shapes_or_scene_table, torch.Tensor) and shapes_or_scene_table.device == seed.device \
            and shapes_or_scene_table.dtype == torch.int64 and shapes_or_scene_table.is_contiguous():
        table = shapes_or_scene_table
    else:
        table = torch.from_numpy(host).to(seed.device)
    src, d2 = _nearest_seed(seed, table, host, 1 if limit == 0 else int(limit or 0))
    if limit == 0:                                                    # the entry's 0 means none: run with 1, keep the seeds
        far = d2 != 0
        src, d2 = src.masked_fill_(far, -1), d2.masked_fill_(far, -1)
    return src, d2


def fill_voids(dem: torch.Tensor, void: torch.Tensor, src, scene_table: torch.Tensor, base: torch.Tensor) -> torch.Tensor:
    """One launch, in place on a flat fp32 device buffer of scenes (a store's lr_dem): dem[p] = dem[scene offset + src[p]]
    where void[p] is set -- the scene's base[scene] where src[p] is -1, or everywhere with src=None -- and dem[p] elsewhere.
    src: `nearest_seed` of the plane `void ^ 1`; scene_table (n, 3) int64 and base (n,) fp32 on the device.  A source that
    is itself a void counts as none, so no value is both read and written."""
    n = dem.numel()
    for name, t, dt in (("dem", dem, torch.float32), ("void", void, torch.uint8), ("src", src, torch.int32), ("base", base, torch.float32),
                        ("scene_table", scene_table, torch.int64)):
        if t is None and name == "src":
            continue
        if t.dtype != dt or not t.is_contiguous() or t.device != dem.device or not t.is_cuda:
            raise ValueError(f"fill_voids: {name} must be a contiguous {dt} tensor on {dem.device}")
        if name in ("void", "src") and t.numel() != n:
            raise ValueError(f"fill_voids: {name} has {t.numel()} elements, dem {n}")
    if scene_table.dim() != 2 or scene_table.shape[1] != 3 or base.numel() != scene_table.shape[0]:
        raise ValueError(f"fill_voids: scene_table {tuple(scene_table.shape)}, base {tuple(base.shape)}")
    _lib.check(_lib.load().jspsr_scene_fill_voids(dem.data_ptr(), void.data_ptr(), None if src is None else src.data_ptr(), n,
                                                  scene_table.data_ptr(), scene_table.shape[0], base.data_ptr(),
                                                  torch.cuda.current_stream(dem.device).cuda_stream), "jspsr_scene_fill_voids")
    return dem


def mask_out(out: torch.Tensor, void_out: torch.Tensor, rows: torch.Tensor, nodata) -> torch.Tensor:
    """One launch, in place on a flat fp32 device buffer: out[rows[r][0] + i] = np.float32(nodata) where
    void_out[rows[r][1] + i] is set, i < rows[r][2]; rows (m, 3) int64 on the device {offset into out, offset into the
    plane, pixels}; a row that leaves either buffer is skipped."""
    if out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("mask_out: out must be a contiguous fp32 tensor on the device")
    if void_out.dtype != torch.uint8 or not void_out.is_contiguous() or void_out.device != out.device:
        raise ValueError(f"mask_out: void_out must be a contiguous uint8 tensor on {out.device}")
    if rows.dtype != torch.int64 or rows.dim() != 2 or rows.shape[1] != 3 or not rows.is_contiguous() or rows.device != out.device:
        raise ValueError(f"mask_out: rows must be a contiguous (m, 3) int64 tensor on {out.device}")
    _lib.check(_lib.load().jspsr_scene_mask_out(out.data_ptr(), out.numel(), void_out.data_ptr(), void_out.numel(), rows.data_ptr(),
                                                rows.shape[0], float(np.float32(nodata)),
                                                torch.cuda.current_stream(out.device).cuda_stream), "jspsr_scene_mask_out")
    return out


def _mask_rows(scenes, indices, offsets) -> torch.Tensor:
    """The device table of `mask_out` for a predict_scenes call, kept with the store per index list (the offsets follow
    from it) as `_table` keeps its tables: int64 rows uploaded as pairs of int32."""
    key = ("mask_out", tuple(int(s) for s in indices))

    def build():
        starts = np.concatenate([[0], np.cumsum([h * w for h, w in scenes.shapes])])
        rows = np.array([[offsets[pos], starts[s], scenes.shapes[s][0] * scenes.shapes[s][1]] for pos, s in enumerate(key[1])],
                        dtype=np.int64)
        return (rows.view(np.int32),), None
    return _store_table(scenes, key, build)[0].view(torch.int64)


def _result(scenes, indices, offsets, buffer, mask_voids) -> "SceneRasters":
    """predict_scenes' end: for a store that holds voids one more launch writes its no-data value into the result."""
    if mask_voids and getattr(scenes, "void_out", None) is not None and sum(scenes.void_counts) > 0:
        mask_out(buffer, scenes.void_out, _mask_rows(scenes, indices, offsets), scenes.nodata)
    return SceneRasters(buffer, offsets, [tuple(scenes.shapes[s]) for s in indices], [scenes.ids[s] for s in indices])


def _model_name(model, model_name):
    return str(model_name or getattr(model, "name", None) or type(model).__module__.rsplit(".", 1)[-1]).lower()


def _model_inputs(name, scenes, input_data):
    """(concat, positions of prepare's outputs to pass on), as `data.batch_pair` chooses a model's inputs."""
    kinds = _input_kinds(scenes)
    if name == "completionformer":
        raise NotImplementedError("the completionformer split input is not built")
    want = kinds if input_data is None else ["lr_dem"] + [k for k in CONCAT_ORDER[1:] if k in input_data]
    missing = [k for k in want if k not in kinds]
    if missing:
        raise ValueError(f"input_data asks for {missing}, the store holds {kinds}")
    if name in {"jspsr", "lrru"}:
        return False, [kinds.index(k) for k in want]
    if want != kinds:
        raise ValueError(f"input_data asks for {want}, the store holds {kinds}: a concatenated input takes every kind")
    return True, [0]


class SceneRasters:
    """What `predict_scenes` returns: `buffer` flat fp32 on the device, and per scene, in the order the scenes were named,
    `offsets` (elements into the buffer), `shapes` and `ids`."""

    def __init__(self, buffer, offsets, shapes, ids):
        self.buffer, self.offsets, self.shapes, self.ids = buffer, offsets, shapes, ids

    def rasters(self) -> dict:
        """{scene id: (H, W) float32 numpy array}: one device-to-host copy.  `list(rasters().values())` over a whole store
        is what `summary.summarise` takes as `predictions`."""
        host = self.buffer.cpu().numpy()
        return {sid: host[o:o + h * w].reshape(h, w).copy() for sid, o, (h, w) in zip(self.ids, self.offsets, self.shapes)}


@torch.no_grad()
def predict_scenes(model, scenes, indices: Sequence[int] | None = None, *, batch_size: int = 1, pad=0,
                   model_name: str | None = None, input_data: dict | None = None, metres: bool = True,
                   tta=None, tile=None, overlap: int | None = None, trim: int = 0, window_tta=None,
                   mask_voids: bool = True) -> SceneRasters:
    """Whole scenes through the model: `model.eval()`, no gradients; the scenes are grouped by shape in index order and,
    per group, each batch runs prepare -> forward -> finish (two launches around the forward, written straight into the
    result's buffer).  No host synchronisation anywhere in the pass.

    scenes: an `InferenceScenes`, or a `data.DeviceScenes` (its hr_dem is not read).  pad: the mirror border in pixels, or
    "pow2" for `tiles.cal_pad` (the reference's rule; it asserts that both sides get the same border).  The frame is
    extended to a multiple of `model.size_multiple` (JSPSR 8, LRRU 16, EDSR 1).  model_name / input_data choose the inputs
    as `data.batch_pair` does: JSPSR / LRRU get [lr_dem, image, mask, canopy, coord] as far as input_data names them (None:
    every kind of the store), any other model the concatenated tensor.  metres=False leaves the network's range.

    tta: None, or the self-ensemble (K14): "d4" or a sequence of D4 elements (`d4_elements`).  Every scene is run in each of
    the orientations -- transformed, then padded -- and the predictions, carried back, are averaged in fp32 in the order
    of the elements before the metre conversion (`prepare_d4`, `finish_mean`).  The variants ride the batch dimension:
    `batch_size` bounds the SAMPLES of a forward.  A square scene's elements share one frame shape; a rectangular scene's
    quarter turns have the transposed one, so its two rot90 parities are separate forwards.

    tile: None, or the tiled pass (K15): k or (kh, kw), a multiple of `model.size_multiple`.  A scene with both sides within
    the tile runs as above, untiled.  Every other scene is covered by `plan_cover(H, W, tile, overlap, trim)` -- overlap
    defaults to a quarter of the smaller tile side -- and its windows, listed in scene order and row-major, run in forwards
    of `batch_size` windows (windows of different scenes and shapes share a batch); the predictions are merged in metres
    with the cover's ramp weights, one launch per group of equally shaped scenes.  pad must be 0 for such a scene.  Each
    tile is a forward of its own: channel-gate statistics are per tile and the convolutions see zeros past a tile's edge,
    as in the reference's tiled validation; `trim` drops that many pixels on the tile sides that face another tile.
    ValueError for a scene with exactly one side below its tile side (pass a rectangular tile); NotImplementedError
    together with `tta`.

    window_tta: None, or the self-ensemble per window (K16), with `tile`: what `tta` takes.  This is not a tiled `tta` --
    that would cover the TRANSFORMED scene, and a cover's origins are not mirror-symmetric: the upright cover stays, and
    every window is run in each orientation (`prepare_windows_d4`).  A scene within the tile runs as with tta=window_tta:
    its one window is the scene.  The windows of the other scenes go in chunks of nb = max(1, batch_size // m) windows, m
    the largest set of elements that share a shape -- all of them for a square tile, the larger rot90 parity for a
    rectangular one -- and each set in forwards of max(1, batch_size // nb) elements, even rot90 before odd, element-major,
    so that `batch_size` still bounds the samples of a forward.  Per chunk one launch carries the predictions back and
    averages them in fp32 in the order of the elements (`mean_windows`); the fp32 mean tiles are then merged as above, the
    mean before the metres as with `tta`.  window_tta=[(0, False, False)] gives the bits of the plain tiled pass.
    ValueError without `tile` and together with `tta`.

    mask_voids (K17): a store built with `nodata` was filled at construction, so every path above reads finite values.  With
    mask_voids=True one more launch at the end, for all scenes of the call and either `metres`, writes np.float32(scenes.nodata)
    into the result wherever `scenes.void_out` is set; False returns the filled prediction.  A store without `nodata`, or
    with no void in it, launches nothing more."""
    window_elements = None if window_tta is None else d4_elements(window_tta)
    if window_elements is not None and tile is None:
        raise ValueError("predict_scenes: window_tta transforms the windows of a tiled pass; give tile (or use tta)")
    if window_elements is not None and tta is not None:
        raise ValueError("predict_scenes: window_tta together with tta; the scene-level ensemble of a tiled pass is not built")
    elements = None if tta is None else d4_elements(tta)
    if tile is not None and elements is not None:
        raise NotImplementedError("predict_scenes: tile together with tta (a windowed prepare_d4) is not built")
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    indices = list(range(len(scenes))) if indices is None else [int(i) for i in indices]
    if not indices:
        raise ValueError("predict_scenes: no scenes")
    concat, take = _model_inputs(_model_name(model, model_name), scenes, input_data)
    multiple = int(getattr(model, "size_multiple", 1))
    tiled_groups = {}
    if tile is not None:
        kh, kw = _tile_sides(tile)
        if kh % multiple or kw % multiple:
            raise ValueError(f"predict_scenes: a tile of {kh} x {kw} is not a multiple of the model's {multiple}")
        overlap = min(kh, kw) // 4 if overlap is None else int(overlap)
    groups = {}
    for pos, s in enumerate(indices):
        groups.setdefault(tuple(scenes.shapes[s]), []).append(pos)
    if tile is not None:
        for (h, w) in groups:
            if (h < kh) != (w < kw) and not (h <= kh and w <= kw):
                raise ValueError(f"predict_scenes: a {h} x {w} scene has one side below the {kh} x {kw} tile; pass a rectangular "
                                 f"tile=(kh, kw) that fits")
        tiled_groups = {shape: m for shape, m in groups.items() if not (shape[0] <= kh and shape[1] <= kw)}
        if tiled_groups:
            if pad != 0:
                raise ValueError(f"predict_scenes: pad must be 0 for a tiled scene, got {pad!r}")
            covers = {shape: plan_cover(shape[0], shape[1], (kh, kw), overlap, trim) for shape in tiled_groups}  # raises here
    order, offsets, total = [], [0] * len(indices), 0
    for (h, w), members in groups.items():
        total = (total + 3) // 4 * 4                          # a group starts 16-byte aligned
        for pos in members:
            offsets[pos] = total
            total += h * w
        order += members
    table = _table(scenes, [indices[pos] for pos in order])
    buffer = torch.empty(total, dtype=torch.float32, device=scenes.device)
    model.eval()
    if elements is not None:
        _predict_tta(model, scenes, indices, elements, groups, offsets, buffer, batch_size, pad, multiple, concat, take, metres)
        return _result(scenes, indices, offsets, buffer, mask_voids)
    if tiled_groups:
        tiled = sorted(pos for members in tiled_groups.values() for pos in members)
        if window_elements is not None:
            _predict_tiled_tta(model, scenes, indices, tiled, tiled_groups, covers, offsets, buffer, batch_size, concat, take,
                               metres, window_elements)
        else:
            _predict_tiled(model, scenes, indices, tiled, tiled_groups, covers, offsets, buffer, batch_size, concat, take, metres)
    if window_elements is not None:                               # the scenes within the tile: their one window is the scene
        whole = {shape: members for shape, members in groups.items() if shape not in tiled_groups}
        _predict_tta(model, scenes, indices, window_elements, whole, offsets, buffer, batch_size, pad, multiple, concat, take, metres)
        return _result(scenes, indices, offsets, buffer, mask_voids)
    at = 0
    for (h, w), members in groups.items():
        if (h, w) in tiled_groups:
            at += len(members)
            continue
        n = T.cal_pad(h, w) if pad == "pow2" else int(pad)
        for lo in range(0, len(members), batch_size):
            B = min(batch_size, len(members) - lo)
            rows = table[at + lo:at + lo + B]
            inputs, frame = _prepare(scenes, rows, h, w, n, multiple, concat)
            pred = model(*[inputs[i] for i in take])
            o = offsets[members[lo]]
            _finish(pred, rows, scenes, frame, metres, buffer[o:o + B * h * w])
        at += len(members)
    return _result(scenes, indices, offsets, buffer, mask_voids)


def _get(p, name, default=None):
    return p.get(name, default) if isinstance(p, dict) else getattr(p, name, default)


def _as_u8(a, name):
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a
    b = a.astype(np.uint8)
    if not np.array_equal(b, a):
        raise ValueError(f"upscale_dem: {name} holds values that are not whole numbers 0..255")
    return b


def upscale_dem(model, sample: dict, p):
    """The reference's `upscale_dem(model, sample, p)` (utils/utils.py:1556-1654) -> (y, t_infer_ms, m_infer_MB).

    sample: HWC numpy arrays "lr_dem" and, optionally, "image" and "mask" (the mask_channel selection applied), plus
    `sample["meta"]["base"]` when `p.relative` (KeyError without it, as in the reference).  p (attributes or keys):
    mask_channel, relative, tensor_kwargs {min, max, log, scale_mask, image_range}, model_name, input_data.  The elevation
    range tensor_kwargs min / max is required (ValueError without it).  As in the reference, the inputs are the rasters
    the SAMPLE holds; `input_data` does not choose them.  The reference reads it only for the channel counts of the
    concatenated tensor, so here, for a model with a concatenated input, an input_data whose image / mask channels differ
    from the sample's is a ValueError; for JSPSR / LRRU it is not read.
    The border is `cal_pad` of the DEM, with the reference's assertion that both sides get the same one.  The padded
    frame must be a multiple of `model.size_multiple`, otherwise ValueError -- the reference would fail inside the model's
    concat; `predict_scenes` extends such frames.  The model runs as it is handed over (the reference does not call
    `eval()` either) under no_grad.
    y: (H, W, 1) float32 in the network's range, unclamped, the padding removed.  t_infer: the forward alone, between two
    events and followed by a synchronisation, in ms.  m_infer: `torch.cuda.max_memory_allocated` after a reset of the
    peak, in MB.
    Models other than JSPSR / LRRU get the concatenated input [lr_dem | image | mask], as `data.batch_pair` builds it; the
    reference's own `else` branch fills that tensor and then passes the list [dem, img, msk] instead (:1628), which no
    such model accepts."""
    dem = np.asarray(sample["lr_dem"])
    if dem.ndim != 3 or dem.shape[2] != 1:
        raise ValueError(f"upscale_dem: lr_dem must be (H, W, 1), got {dem.shape}")
    H, W = dem.shape[:2]
    pad = T.cal_pad(H, W)
    multiple = int(getattr(model, "size_multiple", 1))
    if (H + 2 * pad) % multiple or (W + 2 * pad) % multiple:
        raise ValueError(f"upscale_dem: a {H} x {W} scene pads to {H + 2 * pad} x {W + 2 * pad}, not a multiple of {multiple}; "
                         f"predict_scenes extends the frame to one")
    relative = bool(_get(p, "relative", False))
    base = sample["meta"]["base"] if relative else 0.0
    kw = _get(p, "tensor_kwargs") or {}
    if kw.get("min") is None or kw.get("max") is None:
        raise ValueError("upscale_dem: p.tensor_kwargs must give the elevation range, min and max")
    name = _model_name(model, _get(p, "model_name"))
    input_data = _get(p, "input_data")
    if name not in {"jspsr", "lrru"} and input_data is not None:
        for k in ("image", "mask"):
            have = np.asarray(sample[k]).shape[2] if k in sample else 0
            if int(input_data.get(k, 0)) != have:
                raise ValueError(f"upscale_dem: input_data gives {k} {input_data.get(k, 0)} channels, the sample holds {have}")
    device = next(model.parameters()).device
    scenes = InferenceScenes([np.ascontiguousarray(dem, dtype=np.float32)],
                             image=[np.ascontiguousarray(_as_u8(sample["image"], "image"))]
                             if "image" in sample else None,
                             mask=[np.ascontiguousarray(_as_u8(sample["mask"], "mask"))] if "mask" in sample else None,
                             relative=relative, elev_min=kw.get("min"), elev_max=kw.get("max"), elev_log=kw.get("log", False),
                             scale_mask=kw.get("scale_mask", False), mask_channel=_get(p, "mask_channel"),
                             image_range=kw.get("image_range"), device=device, base=[base] if relative else None)
    concat = name not in {"jspsr", "lrru"}
    with torch.no_grad():
        inputs, frame = prepare(scenes, [0], pad, 1, concat)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.reset_peak_memory_stats(device)
        start.record()
        y = model(*inputs)
        stop.record()
        torch.cuda.current_stream(device).synchronize()
        t_infer = start.elapsed_time(stop)
        m_infer = torch.cuda.max_memory_allocated(device) / 1024 / 1024
        y = finish(y, scenes, [0], frame, metres=False)
    return y[0].cpu().numpy()[..., None], t_infer, m_infer
