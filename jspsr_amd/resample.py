"""Rasters resampled to a finer grid on the device (K25, csrc/resample.hip): `F.interpolate(size=, mode="bicubic" |
"bilinear", align_corners=False)` for single-channel fp32 rasters, a list of different shapes in ONE launch.

The reference resizes a smaller input DEM bicubically before it scores it (evaluation/evaluate_utils.py:331-332), and real
stores hold their DEM at its own resolution (30 m tiles under 8 m imagery: a ratio of 3.75).  Here that resize is

    dst, dst_table = resample_rasters(src, src_table, dst_shapes)          # flat stores, rasters of any shapes
    y = resize(x, (H, W))                                                  # (B, C, h, w) -> (B, C, H, W)

and `InferenceScenes(..., lr_resample="bicubic")` / `DeviceScenes(..., lr_resample=)` take lr_dem on its own grid and
bring it to the grid of the other rasters at construction.  Upsampling only: no prefilter is built.

Numerics.  The tap weights of an axis are made on the host in double from a coordinate taken apart in integers and
rounded to fp32 once (`axis_taps`, jspsr_resample_axis); the kernel interpolates the differences to the centre tap in
single fp32 roundings, so its error follows the relief under the taps and not the elevation: on terrain at 1500 m it stays
below an ulp of the result where torch's fp32 bicubic is 13 ulp from its own fp64 result.  tests/resample_ref.py restates
both in numpy; the kernel has its bits, on every run and whatever rasters share the call.

A bicubic baseline row for `summary.summarise(baselines=...)`, from the coarse rasters alone:

    sizes = [a.size for a in lr_native]                                      # lr_native: per-scene (h, w) fp32 metres
    coarse = torch.from_numpy(np.concatenate([a.reshape(-1) for a in lr_native])).to(scenes.device)
    table = [(sum(sizes[:i]), *a.shape) for i, a in enumerate(lr_native)]
    bicubic, _ = resample_rasters(coarse, table, scenes.shapes)              # flat, in the store's layout
    rows = summarise(scenes, predictions, baselines={"Bicubic": bicubic}, value_max=933, patch_size=128)

The other direction (K26, csrc/area.hip): HWC uint8 rasters held FINER than their scene -- image, mask, canopy -- brought to
the scene's grid by their exact area mean, a list of different shapes and one channel count in ONE launch:

    dst, dst_table = area_rasters(src, src_table, channels, dst_shapes)    # mode="area" | "majority" (one-hot masks)
    y = area_resize(x, (H, W))                                             # (B, h, w, C) uint8 -> (B, H, W, C)

and `InferenceScenes(..., guide_resample="area")` / `DeviceScenes(..., guide_resample=)` take the three kinds on grids of
their own.  Integers throughout (`area_axis`, jspsr_area_axis: the overlaps of output and source pixels as weights; 64-bit
sums; a division corrected by its remainder): tests/area_ref.py restates it in numpy int64 and the kernel has its bytes.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Sequence

import numpy as np
import torch

from . import _lib

MODES = {"bicubic": 0, "bilinear": 1}                 # JSPSR_RESAMPLE_* (include/jspsr_hip.h)
ROW = 8                                               # int64 words per raster of the kernel's table
_TAPS = {}                                            # (mode, axes, device) -> _Uploaded((first, weight bits)), {axis: offset}
_TABLES = {}                                          # (rows as bytes, device) -> _Uploaded((rows as int32 pairs,))


def _mode(mode) -> int:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    return MODES[mode]


@functools.lru_cache(maxsize=512)
def _axis(h: int, H: int, mode: str):
    first = np.empty(H, dtype=np.int32)
    weights = np.empty((H, 4), dtype=np.float32)
    _lib.check(_lib.load().jspsr_resample_axis(h, H, MODES[mode], first.ctypes.data, weights.ctypes.data), "jspsr_resample_axis")
    first.setflags(write=False)
    weights.setflags(write=False)
    return first, weights


def axis_taps(h: int, H: int, mode: str = "bicubic"):
    """The taps of one axis, output length H over a source of h (host code of the library, no GPU) -> (first (H,) int32,
    weights (H, 4) fp32), read-only and cached: tap k of output Y is source index clip(first[Y] + k, 0, h - 1).  bicubic:
    four taps from i - 1; bilinear: two taps from i, weights[:, 2:] zero.  ValueError for H < h: downsampling is not built."""
    _mode(mode)
    for name, v in (("h", h), ("H", H)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError(f"axis_taps: {name} must be a whole number >= 1, got {v!r}")
    if int(H) < int(h):
        raise ValueError(f"axis_taps: {h} -> {H} is a downsampling: it needs a prefilter and is not built")
    return _axis(int(h), int(H), mode)


def _device_taps(axes, mode, device):
    """The device copy of the axis tables `axes` (sorted distinct (h, H)) back to back -> (first, weights, {axis: offset}),
    cached per (mode, axes, device) as `infer._device_maps` caches `frame_maps`: a repeated call uploads nothing."""
    from . import infer

    def build():
        taps = [axis_taps(h, H, mode) for h, H in axes]
        offs = np.concatenate([[0], np.cumsum([H for _, H in axes])])
        return ((np.concatenate([f for f, _ in taps]), np.concatenate([w.reshape(-1) for _, w in taps]).view(np.int32)),
                {a: int(o) for a, o in zip(axes, offs)})
    (first, wbits), offsets = infer._cached(_TAPS, (mode, axes, str(device)), device, build)
    return first, wbits, offsets


def _host_rows(src_table, dst_shapes):
    src_table = src_table.detach().cpu().numpy() if isinstance(src_table, torch.Tensor) else src_table
    st = np.asarray(src_table, dtype=np.int64)
    ds = np.asarray([tuple(int(v) for v in s) for s in dst_shapes], dtype=np.int64)
    if st.ndim != 2 or st.shape[1] != 3 or st.shape[0] == 0:
        raise ValueError(f"resample_rasters: src_table is (n, 3) rows {{offset, h, w}}, got shape {st.shape}")
    if ds.shape != (st.shape[0], 2):
        raise ValueError(f"resample_rasters: {st.shape[0]} rasters, dst_shapes has shape {ds.shape}")
    return st, ds


def resample_rasters(src: torch.Tensor, src_table, dst_shapes: Sequence, mode: str = "bicubic", clamp=None, void=None):
    """One launch: the rasters of the flat fp32 device buffer `src` named by `src_table` -- host rows {offset, h, w}, such
    as a store's scene table -- each resampled to its (H, W) of `dst_shapes` -> (dst, dst_table[, dst_void]).  dst: flat
    fp32 on the device, the results back to back; dst_table: (n, 3) int64 numpy rows {offset, H, W} into it.
    clamp: per-raster [lo, hi], (n, 2) fp32 (a device tensor, or host values that are uploaded): out < lo ? lo : (out > hi ?
    hi : out), NaN kept -- bicubic overshoots a step edge, and a clamp to the source's own range keeps a result inside it.
    void: flat uint8 device plane in src's layout; dst_void (dst's layout) is then returned too, an output pixel taking the
    byte of its centre tap, source pixel (iy, ix) clamped to the raster, i the floor of its coordinate.  A void that still holds NaN reaches the outputs within
    two source pixels of it and no others.
    ValueError for a shape that downsamples (H < h or W < w).  No host synchronisation; what the launch reads is uploaded
    once per set of shapes and kept."""
    from . import infer
    m = _mode(mode)
    if src.dtype != torch.float32 or src.dim() != 1 or not src.is_contiguous() or not src.is_cuda:
        raise ValueError(f"resample_rasters: src must be a flat contiguous fp32 tensor on the device, got {src.dtype} "
                         f"{tuple(src.shape)} on {src.device}")
    st, ds = _host_rows(src_table, dst_shapes)
    n = len(st)
    for k in range(n):
        (o, h, w), (H, W) = st[k], ds[k]
        if h < 1 or w < 1 or o < 0 or o + h * w > src.numel():
            raise ValueError(f"resample_rasters: raster {k} {{offset {o}, {h} x {w}}} is not inside src ({src.numel()} elements)")
        if H < h or W < w:
            raise ValueError(f"resample_rasters: raster {k}: {h} x {w} -> {H} x {W} is a downsampling: it needs a prefilter and is "
                             f"not built")
    axes = tuple(sorted({(int(st[k, 1]), int(ds[k, 0])) for k in range(n)} | {(int(st[k, 2]), int(ds[k, 1])) for k in range(n)}))
    first, wbits, at = _device_taps(axes, mode, src.device)
    rows = np.zeros((n, ROW), dtype=np.int64)
    rows[:, 0:3] = st
    rows[:, 4:6] = ds
    rows[1:, 3] = np.cumsum(ds[:, 0] * ds[:, 1])[:-1]
    rows[:, 6] = [at[(int(st[k, 1]), int(ds[k, 0]))] for k in range(n)]
    rows[:, 7] = [at[(int(st[k, 2]), int(ds[k, 1]))] for k in range(n)]
    total = int(np.sum(ds[:, 0] * ds[:, 1]))
    (table,), host_rows = infer._cached(_TABLES, (rows.tobytes(), str(src.device)), src.device, lambda: ((rows.view(np.int32),), rows))
    if clamp is not None:
        if not isinstance(clamp, torch.Tensor):
            pinned = torch.empty((n, 2), dtype=torch.float32, pin_memory=True)
            pinned.numpy()[...] = np.asarray(clamp, dtype=np.float32).reshape(n, 2)
            clamp = pinned.to(src.device, non_blocking=True)
        if clamp.dtype != torch.float32 or tuple(clamp.shape) != (n, 2) or not clamp.is_contiguous() or clamp.device != src.device:
            raise ValueError(f"resample_rasters: clamp must be a contiguous ({n}, 2) fp32 tensor on {src.device}")
    if void is not None:
        if void.dtype != torch.uint8 or void.dim() != 1 or void.numel() != src.numel() or not void.is_contiguous() \
                or void.device != src.device:
            raise ValueError(f"resample_rasters: void must be a flat contiguous uint8 plane of {src.numel()} elements on {src.device}")
    dst = torch.empty(total, dtype=torch.float32, device=src.device)
    dst_void = torch.empty(total, dtype=torch.uint8, device=src.device) if void is not None else None
    _lib.check(_lib.load().jspsr_resample_forward(
        src.data_ptr(), src.numel(), dst.data_ptr(), total, table.data_ptr(), host_rows.ctypes.data, n, first.data_ptr(),
        wbits.data_ptr(), first.numel(), m, None if clamp is None else clamp.data_ptr(), None if void is None else void.data_ptr(),
        None if void is None else dst_void.data_ptr(), torch.cuda.current_stream(src.device).cuda_stream), "jspsr_resample_forward")
    dst_table = np.ascontiguousarray(rows[:, 3:6])
    return (dst, dst_table) if void is None else (dst, dst_table, dst_void)


def resize(x: torch.Tensor, size, mode: str = "bicubic") -> torch.Tensor:
    """`F.interpolate(x, size=size, mode=mode, align_corners=False)` for a contiguous fp32 (B, C, h, w) device tensor, every
    plane one raster of one launch -> (B, C, H, W).  No clamp (bicubic overshoots, as torch's does)."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"resize: a (B, C, h, w) fp32 tensor on the device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"resize: size is (H, W), got {size!r}") from None
    B, C, h, w = x.shape
    planes = B * C
    if planes < 1:
        raise ValueError("resize: an empty tensor")
    out = []
    x = x.detach().contiguous()
    for lo in range(0, planes, 65535):                                       # the launch takes 65535 rasters
        m = min(65535, planes - lo)
        table = [(k * h * w, h, w) for k in range(m)]
        out.append(resample_rasters(x.view(-1)[lo * h * w:(lo + m) * h * w], table, [(H, W)] * m, mode)[0])
    return (out[0] if len(out) == 1 else torch.cat(out)).view(B, C, H, W)


# ---- K26 (csrc/area.hip): HWC uint8 rasters brought to a coarser grid by their exact area mean

AREA_MODES = {"area": 0, "majority": 1}               # JSPSR_AREA_* (include/jspsr_hip.h)
AREA_ROW = 6                                          # int64 words per raster of the area kernel's table
AREA_SIDE_MAX = 65535                                 # the kernel's weight products are 32-bit
_AREA_TABLES = {}                                     # (rows as bytes, device) -> _Uploaded((rows as int32 pairs,))


def _area_mode(mode) -> int:
    if mode not in AREA_MODES:
        raise ValueError(f"mode must be one of {sorted(AREA_MODES)}, got {mode!r}")
    return AREA_MODES[mode]


@functools.lru_cache(maxsize=512)
def _area_axis(h: int, H: int):
    taps = (h + H - 1) // H + 1
    first, count = np.empty(H, dtype=np.int32), np.empty(H, dtype=np.int32)
    weights = np.empty((H, taps), dtype=np.uint32)
    _lib.check(_lib.load().jspsr_area_axis(h, H, first.ctypes.data, count.ctypes.data, weights.ctypes.data), "jspsr_area_axis")
    for a in (first, count, weights):
        a.setflags(write=False)
    return first, count, weights


def area_axis(h: int, H: int):
    """The area weights of one axis, output length H over a source of h, 1 <= H <= h (host code of the library, no GPU) ->
    (first (H,) int32, count (H,) int32, weights (H, ceil(h / H) + 1) uint32), read-only and cached: output Y covers the
    source pixels first[Y] .. first[Y] + count[Y] - 1 with the integer weights weights[Y, :count[Y]] (the overlap in units
    of 1 / (h H) of the axis; a row sums to h, a source pixel's weights to H), zero past count[Y].  ValueError for H > h:
    upsampling of these rasters is not built."""
    for name, v in (("h", h), ("H", H)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError(f"area_axis: {name} must be a whole number >= 1, got {v!r}")
    if int(H) > int(h):
        raise ValueError(f"area_axis: {h} -> {H} is an upsampling, which is not built")
    if int(h) > AREA_SIDE_MAX:
        raise ValueError(f"area_axis: a source of {h} pixels, the kernel takes sides up to {AREA_SIDE_MAX}")
    return _area_axis(int(h), int(H))


def area_rasters(src: torch.Tensor, src_table, channels: int, dst_shapes: Sequence, mode: str = "area"):
    """One launch (K26): the HWC uint8 rasters of the flat device buffer `src` named by `src_table` -- host rows {offset, h,
    w} in PIXELS, `channels` bytes per pixel (1..16, the same for all) -- each brought to its coarser (H, W) of `dst_shapes`
    -> (dst, dst_table).  dst: flat uint8 on the device, the results back to back; dst_table: (n, 3) int64 numpy rows
    {offset, H, W} in pixels.  Any ratio >= 1 per axis, the extents taken as equal.
    mode "area": the exact area mean per channel, rounded half up -- with the integer overlaps a of `area_axis`,
    floor((sum a_y a_x v + D // 2) / D), D = h w; H == h and W == w gives the input's bytes.  mode "majority", for one-hot
    masks (a non-zero byte counts as 1): the pixel is one-hot at the channel of largest coverage, the lowest index among
    equals, iff that coverage is positive and at least the uncovered rest D - sum_c S_c; otherwise all zeros.
    Integers throughout: tests/area_ref.py restates both in numpy int64 and the output has its bytes, on every run and
    whatever rasters share the call.  ValueError for a shape that is an upsampling (H > h or W > w) or a side above 65535.
    No host synchronisation; the table is uploaded once per set of shapes and kept."""
    from . import infer
    m = _area_mode(mode)
    if isinstance(channels, (bool, np.bool_)) or not isinstance(channels, (int, np.integer)) or not 1 <= int(channels) <= 16:
        raise ValueError(f"area_rasters: channels must be a whole number in 1..16, got {channels!r}")
    C = int(channels)
    if src.dtype != torch.uint8 or src.dim() != 1 or not src.is_contiguous() or not src.is_cuda:
        raise ValueError(f"area_rasters: src must be a flat contiguous uint8 tensor on the device, got {src.dtype} "
                         f"{tuple(src.shape)} on {src.device}")
    src_table = src_table.detach().cpu().numpy() if isinstance(src_table, torch.Tensor) else src_table
    st = np.asarray(src_table, dtype=np.int64)
    ds = np.asarray([tuple(int(v) for v in s) for s in dst_shapes], dtype=np.int64)
    if st.ndim != 2 or st.shape[1] != 3 or st.shape[0] == 0:
        raise ValueError(f"area_rasters: src_table is (n, 3) rows {{offset, h, w}}, got shape {st.shape}")
    if ds.shape != (st.shape[0], 2):
        raise ValueError(f"area_rasters: {st.shape[0]} rasters, dst_shapes has shape {ds.shape}")
    n = len(st)
    if n > 65535:
        raise ValueError(f"area_rasters: {n} rasters, one call takes at most 65535")
    pixels = src.numel() // C
    for k in range(n):
        (o, h, w), (H, W) = st[k], ds[k]
        if h < 1 or w < 1 or o < 0 or o + h * w > pixels:
            raise ValueError(f"area_rasters: raster {k} {{offset {o}, {h} x {w}}} is not inside src ({pixels} pixels of {C} channels)")
        if H < 1 or W < 1:
            raise ValueError(f"area_rasters: raster {k}: {h} x {w} -> {H} x {W} has an empty side")
        if H > h or W > w:
            raise ValueError(f"area_rasters: raster {k}: {h} x {w} -> {H} x {W} is an upsampling, which is not built")
        if h > AREA_SIDE_MAX or w > AREA_SIDE_MAX:
            raise ValueError(f"area_rasters: raster {k} is {h} x {w}, the kernel takes sides up to {AREA_SIDE_MAX}")
    rows = np.zeros((n, AREA_ROW), dtype=np.int64)
    rows[:, 0:3] = st
    rows[:, 4:6] = ds
    rows[1:, 3] = np.cumsum(ds[:, 0] * ds[:, 1])[:-1]
    total = int(np.sum(ds[:, 0] * ds[:, 1]))
    (table,), host_rows = infer._cached(_AREA_TABLES, (rows.tobytes(), str(src.device)), src.device,
                                        lambda: ((rows.view(np.int32),), rows))
    dst = torch.empty(total * C, dtype=torch.uint8, device=src.device)
    _lib.check(_lib.load().jspsr_area_forward(src.data_ptr(), pixels, dst.data_ptr(), total, table.data_ptr(), host_rows.ctypes.data,
                                              n, C, m, torch.cuda.current_stream(src.device).cuda_stream), "jspsr_area_forward")
    return dst, np.ascontiguousarray(rows[:, 3:6])


def area_resize(x: torch.Tensor, size, mode: str = "area") -> torch.Tensor:
    """`area_rasters` for a contiguous (B, h, w, C) uint8 device tensor, every image one raster of one launch ->
    (B, H, W, C)."""
    if x.dim() != 4 or x.dtype != torch.uint8 or not x.is_cuda:
        raise ValueError(f"area_resize: a (B, h, w, C) uint8 tensor on the device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"area_resize: size is (H, W), got {size!r}") from None
    B, h, w, C = x.shape
    if B < 1:
        raise ValueError("area_resize: an empty tensor")
    _area_mode(mode)
    out = []
    x = x.detach().contiguous()
    for lo in range(0, B, 65535):                                            # the launch takes 65535 rasters
        m = min(65535, B - lo)
        table = [(k * h * w, h, w) for k in range(m)]
        out.append(area_rasters(x.view(-1)[lo * h * w * C:(lo + m) * h * w * C], table, C, [(H, W)] * m, mode)[0])
    return (out[0] if len(out) == 1 else torch.cat(out)).view(B, H, W, C)
