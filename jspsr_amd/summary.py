"""The whole-set validation summary on the device (K12, csrc/summary.hip): scene mosaics in metres and the pooled scores
the reference publishes.

Restates the last stage of the reference's `--val` path: `save_prediction_to_disk` (evaluation/evaluate_utils.py:242-271:
clip to [0,1], `descale_data`, `+ base`), `merge_dem(..., p.val_border, method=copyto_add)` (utils/utils.py:914-967,
called at :1272) and `summarise_evaluation` (utils/utils.py:970-1368), which scores the whole validation set twice:
"offline", pooled over all pixels of all scenes (the accuracy table of its ReadMe), and "online", per scene and averaged;
both for the prediction and for every baseline DEM against the ground truth.

    c = ScenePredictions(scenes, 128, 9, border=0.05)
    evaluate(model, TileCropBatches(scenes, 50, 128, 9), criterion, meter, "JSPSR", input_data, collector=c)
    table = summarise(scenes, c, baselines={"COP30": "lr_dem"}, value_max=933, border=0.05, patch_size=128)

The pooled numbers differ from the per-tile meters of `metrics.batch_scores` (K10) by definition: numpy's median is the
mean of the two middle elements (torch.median: the lower one) and numpy's percentile interpolates (kthvalue: one element).
Arithmetic and its departures from numpy / the reference: include/jspsr_hip.h, K12.  GeoTIFF output, drawing and the
richdem slope stay out (drawing stays out; the curves are `error_distribution`, K21); `upscale_dem` and whole-scene inference are in jspsr_amd/infer.py (K13), whose
`predict_scenes(...).rasters()` gives the per-scene metre rasters `summarise` takes as `predictions`.

Scores over valid pixels only (K18): `summarise(..., valid=valid_plane(scenes, nodata))`, `scores_pooled(..., valid=)` and
`pooled_rows(..., valid=)` leave the pixels a uint8 plane in the ground truth's layout masks out of every sum and order
statistic, whatever their values (the -32767 of a `predict_scenes(mask_voids=True)` result, a hole in the ground truth), and
also return how many pixels were scored.  The count is data on the device, so the ranks are formed there: still one call of
16 launches without a host synchronisation.

The error distribution (K21, csrc/errdist.hip): `pooled_histogram` counts the pooled errors inside [lo, hi], rounded to
float16 as the reference stores them, into one exact integer histogram per candidate (35 330 bins for [-5, 5]);
`kde_curves` evaluates the Gaussian kernel density estimate of seaborn's kdeplot from it in fp64; `error_distribution`
does both for the candidates `summarise` takes.  Only the curves leave the card.

Scores by terrain class (K22, csrc/strata.hip): `summarise_by_class(scenes, predictions, labels, class_names, ...)` breaks
`summarise`'s pooled table down by the classes of a uint8 label plane in store layout -- land cover made from the store's
mask with torch operators, or `slope_class_plane(scenes, edges_deg, cell)`, one launch that bins the Sobel slope of the
ground truth against `slope_thresholds`.  `stratified_rows` is the raw call and `scores_by_class` the form for equal-shape
tensors.  Every pass over the pool serves all classes at once (per-class digit histograms in LDS): still one call of 16
launches, whatever the number of classes.  A label of 255 (or any label >= n_classes) belongs to no class.  Not built:
per-candidate label planes, more than 32 classes, an "online" per-scene form.

Device fp32 tensors go through the HIP kernels; host tensors through the same formulas as numpy / torch operators.
"""
from __future__ import annotations

import ctypes
import math
from math import floor
from typing import Sequence

import numpy as np
import torch

from . import _lib
from . import metrics as M
from . import tiles as T

CHUNK = 8192                  # csrc/summary.hip: elements of a segment per workgroup
MAX_CANDIDATES = 8
COLUMNS = ("RMSE", "Median", "NMAD", "LE95", "PSNR")
ROW = COLUMNS + ("median_lo", "median_hi", "mad_lo", "mad_hi", "le95_lo", "le95_hi")
_WIN_WORDS = 4 + 2 * (1 + MAX_CANDIDATES)
_SEG_WORDS = 8


def segment_ranks(n: int):
    """The 0-based ranks and the weight every order statistic of a segment of n elements is read at:
    (median lo, median hi, LE95 lo, LE95 hi, g).  Median: the elements of ranks (n - 1) // 2 and n // 2 (np.median).
    LE95: v = 0.95 (n - 1) in double, l = floor(v), g = v - l, the elements of ranks l and min(l + 1, n - 1), value
    lo + (hi - lo) g (np.percentile(., 95) on a float64 array).  The one place these are formed: the device reads them from
    the segment table."""
    if n < 1:
        raise ValueError(f"segment_ranks: n = {n}")
    v = 0.95 * (n - 1)
    lo = int(floor(v))
    return (n - 1) // 2, n // 2, lo, min(lo + 1, n - 1), v - lo


def _row_host(e: np.ndarray, value_max: float) -> np.ndarray:
    """One output row from a float32 error vector, as numpy operators."""
    n = e.size
    m0, m1, l0, l1, g = segment_ranks(n)
    with np.errstate(all="ignore"):
        srt = np.sort(e)
        med = np.float32((srt[m0] + srt[m1]) * np.float32(0.5))
        d = np.sort(np.abs(e - med))
        mad = np.float32((d[m0] + d[m1]) * np.float32(0.5))
        a = np.sort(np.abs(e))
        le = np.float32(float(a[l0]) + (float(a[l1]) - float(a[l0])) * g)
        rm = math.sqrt(float(np.sum(e.astype(np.float64) ** 2)) / n)
        psnr = 20.0 * np.log10(np.float64(value_max) / np.float64(rm))          # +inf at rm == 0
        row = np.array([rm, med, np.float32(1.4826 * float(mad)), le, psnr, srt[m0], srt[m1], d[m0], d[m1], a[l0], a[l1]],
                       dtype=np.float32)
    if np.isnan(e).any():
        row[:5] = np.nan
    return row


def _nan_row() -> np.ndarray:
    return np.full(len(ROW), np.nan, dtype=np.float32)


def _check_pool(what, cands, gt, windows, valid):
    """The argument checks `pooled_rows` and `pooled_histogram` share: buffers, validity plane, every window inside its
    buffers.  -> the number of pooled elements."""
    n_cand = len(cands)
    if not 1 <= n_cand <= MAX_CANDIDATES:
        raise ValueError(f"{what}: {n_cand} candidates, 1..{MAX_CANDIDATES} are taken")
    bufs = [gt] + list(cands)
    if any(b.dtype != torch.float32 or b.dim() != 1 or not b.is_contiguous() for b in bufs):
        raise ValueError(f"{what}: flat contiguous float32 buffers")
    if len({b.device for b in bufs}) != 1:
        raise ValueError(f"{what}: buffers on several devices")
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8 or valid.dim() != 1 or not valid.is_contiguous():
            raise ValueError(f"{what}: valid must be a flat contiguous uint8 tensor")
        if valid.numel() != gt.numel():
            raise ValueError(f"{what}: valid has {valid.numel()} elements, the ground truth {gt.numel()}")
        if valid.device != gt.device:
            raise ValueError(f"{what}: valid on {valid.device}, the ground truth on {gt.device}")
    total = 0
    for sg, h, w, g_, cs in windows:
        if h <= 0 or w <= 0:
            raise ValueError(f"{what}: an empty window ({h} x {w})")
        if len(cs) != n_cand:
            raise ValueError(f"{what}: a window names {len(cs)} candidates, {n_cand} were given")
        for (off, pitch), b in zip([g_] + list(cs), bufs):
            if off < 0 or pitch < 0 or off + (h - 1) * pitch + w > b.numel():
                raise ValueError(f"{what}: window {h} x {w} at {off} (pitch {pitch}) leaves its buffer of {b.numel()}")
        total += h * w
    return total


def _window_table(windows, keep_segment: bool) -> np.ndarray:
    """The (n, _WIN_WORDS) int64 window rows the pooled kernels read (csrc/pooled_read.h): segment (0 unless keep_segment),
    h, w, the running offset of the window's first element in e, {offset, pitch} of gt and of each candidate; the slots of
    candidates not given stay 0."""
    tab = np.zeros((len(windows), _WIN_WORDS), dtype=np.int64)
    e_off = 0
    for i, (sg, h, w, (go, gp), cs) in enumerate(windows):
        tab[i, :6] = (sg if keep_segment else 0, h, w, e_off, go, gp)
        for c, (co, cp) in enumerate(cs):
            tab[i, 6 + 2 * c: 8 + 2 * c] = (co, cp)
        e_off += h * w
    return tab


def _upload(tab: np.ndarray, dev) -> torch.Tensor:
    """One stream-ordered upload from a pinned buffer that is never written again."""
    host = torch.empty(tab.shape, dtype=torch.int64, pin_memory=True)
    host.numpy()[...] = tab
    return host.to(dev, non_blocking=True)


def _cand_arrays(cands):
    """-> the candidates' (pointer array, numel array) as the C entries take them."""
    n = len(cands)
    return (ctypes.c_void_p * n)(*[c.data_ptr() for c in cands]), (ctypes.c_longlong * n)(*[c.numel() for c in cands])


def _window_index(h, w, off, pitch):
    return off + np.arange(h)[:, None] * pitch + np.arange(w)[None, :]


def _gather_plane(plane: np.ndarray, windows):
    """A plane in gt's layout through a window list -> one flat array per window."""
    return [plane[_window_index(h, w, go, gp)].reshape(-1) for _, h, w, (go, gp), _ in windows]


def _gather_errors(c_np: np.ndarray, g_np: np.ndarray, windows, c: int):
    """Candidate c's cand - gt through a window list -> one flat array per window (the fp32 subtraction; the callers
    concatenate and then `astype(np.float32, copy=False)`)."""
    with np.errstate(invalid="ignore"):                         # inf - inf at an element that is not scored
        return [(c_np[_window_index(h, w, *cs[c])] - g_np[_window_index(h, w, go, gp)]).reshape(-1)
                for _, h, w, (go, gp), cs in windows]


def pooled_rows(cands: Sequence[torch.Tensor], gt: torch.Tensor, windows: Sequence[tuple], n_segments: int, value_max: float,
                valid: torch.Tensor | None = None):
    """The raw table call.  cands: 1..8 flat fp32 buffers, gt one, all on one device; windows: (segment, h, w, (gt offset,
    gt pitch), [(offset, pitch) per candidate]) in elements -- crops are read in place; a segment pools its windows in the
    order given.  -> (n_cand, n_segments, 11) fp32 tensor, columns `ROW`, on the buffers' device.  No host
    synchronisation on the device path (K12(b): one call, 16 launches).
    valid: a flat contiguous uint8 tensor of gt.numel() elements on gt's device, read at gt's offsets and pitches; an
    element is scored iff its byte is non-zero, for every candidate alike (K18: still one call, 16 launches, no
    synchronisation).  -> (rows, counts): rows as above, counts an int64 (n_segments,) tensor on the device, the elements
    scored per segment; a segment with none has a NaN row and count 0."""
    n_cand = len(cands)
    _check_pool("pooled_rows", cands, gt, windows, valid)
    if n_segments < 1 or not windows:
        raise ValueError("pooled_rows: no windows or no segments")
    order = sorted(range(len(windows)), key=lambda i: windows[i][0])          # stable: a segment keeps its window order
    seg_n = [0] * n_segments
    for sg, h, w, g_, cs in windows:
        if not 0 <= sg < n_segments:
            raise ValueError(f"pooled_rows: segment {sg} of {n_segments}")
        seg_n[sg] += h * w
    if min(seg_n) == 0:
        raise ValueError("pooled_rows: a segment without windows")
    total = sum(seg_n)
    windows = [windows[i] for i in order]                         # a segment's windows back to back
    if gt.is_cuda:
        return _pooled_device(cands, gt, windows, seg_n, total, value_max, valid)
    out = np.empty((n_cand, n_segments, len(ROW)), dtype=np.float32)
    g_np = gt.numpy()
    ends = np.cumsum(np.bincount([wdw[0] for wdw in windows], minlength=n_segments))

    def per_segment(parts):                                       # one flat array per window -> one per segment
        return [np.concatenate(parts[a:b]) for a, b in zip([0] + list(ends[:-1]), ends)]

    keep = None
    if valid is not None:
        keep = [k != 0 for k in per_segment(_gather_plane(valid.numpy(), windows))]
    for c, cand in enumerate(cands):
        parts = per_segment(_gather_errors(cand.numpy(), g_np, windows, c))
        for sg in range(n_segments):
            e = parts[sg].astype(np.float32, copy=False)
            if keep is not None:
                e = e[keep[sg]]
            out[c, sg] = _row_host(e, value_max) if e.size else _nan_row()
    if keep is not None:
        return torch.from_numpy(out), torch.tensor([int(k.sum()) for k in keep], dtype=torch.int64)
    return torch.from_numpy(out)


def _pooled_device(cands, gt, windows, seg_n, total, value_max, valid=None):
    n_cand, n_seg, n_win = len(cands), len(seg_n), len(windows)
    seg = np.zeros((n_seg, _SEG_WORDS), dtype=np.int64)
    start = chunk = 0
    for sg, n in enumerate(seg_n):
        m0, m1, l0, l1, g = segment_ranks(n)
        seg[sg] = (start, n, chunk, m0, m1, l0, l1, np.float64(g).view(np.int64))
        start += n
        chunk += (n + CHUNK - 1) // CHUNK
    lib = _lib.load()
    masked = valid is not None
    nbytes = (lib.jspsr_summary_valid_workspace_bytes if masked else lib.jspsr_summary_workspace_bytes)(n_cand, n_seg, total, chunk)
    if nbytes == 0:
        raise ValueError(f"pooled_rows: {n_cand} candidates, {n_seg} segments, {total} pooled elements: not a size K12 takes "
                         "(fewer than 2^32 elements per call)")
    dev = gt.device
    table = _upload(np.concatenate((_window_table(windows, True).reshape(-1), seg.reshape(-1))), dev)   # windows, then segments: one table
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((n_cand, n_seg, len(ROW)), dtype=torch.float32, device=dev)
    ptrs, numel = _cand_arrays(cands)
    if masked:
        counts = torch.empty(n_seg, dtype=torch.int64, device=dev)
        _lib.check(lib.jspsr_summary_valid_forward(ptrs, numel, n_cand, gt.data_ptr(), gt.numel(), valid.data_ptr(), valid.numel(),
                                                   table.data_ptr(), n_win, table.data_ptr() + n_win * _WIN_WORDS * 8, n_seg, total,
                                                   chunk, float(value_max), out.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream),
                   "jspsr_summary_valid_forward")
        return out, counts
    _lib.check(lib.jspsr_summary_forward(ptrs, numel, n_cand, gt.data_ptr(), gt.numel(), table.data_ptr(), n_win,
                                         table.data_ptr() + n_win * _WIN_WORDS * 8, n_seg, total, chunk, float(value_max),
                                         out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "jspsr_summary_forward")
    return out


def scores_pooled(cands, gt, segments=None, value_max: float = 1.0, valid=None):
    """Pooled scores of equal-shape tensors, e.g. a 4096 x 4096 scene from `tiling.sharded_forward_owned` against its
    target.  cands: a tensor or a list of up to 8, each of gt's shape (..., H, W), fp32 metres.  segments: None pools
    everything into one segment; otherwise a list of segments, each a list of windows (plane, y0, x0, h, w) over the
    tensors flattened to (planes, H, W).  value_max: the numerator of PSNR = 20 log10(value_max / RMSE).
    -> (n_cand, n_segments, 11) fp32 tensor on the inputs' device, columns `ROW`; no host synchronisation.
    valid: a bool or uint8 tensor of gt's shape on gt's device; only the pixels where it is set are scored (K18).
    -> (rows, counts) as `pooled_rows` gives them."""
    cands = [cands] if isinstance(cands, torch.Tensor) else list(cands)
    if gt.dim() < 2 or any(c.shape != gt.shape for c in cands):
        raise ValueError(f"scores_pooled: equal (..., H, W) tensors, got {[tuple(c.shape) for c in cands]} / {tuple(gt.shape)}")
    H, W = gt.shape[-2:]
    planes = gt.numel() // (H * W) if H * W else 0
    if segments is None:
        segments = [[(p, 0, 0, H, W) for p in range(planes)]]
    windows = []
    for sg, wins in enumerate(segments):
        for p, y0, x0, h, w in wins:
            if not (0 <= p < planes and 0 <= y0 and 0 <= x0 and y0 + h <= H and x0 + w <= W):
                raise ValueError(f"scores_pooled: window {(p, y0, x0, h, w)} leaves the ({planes}, {H}, {W}) tensor")
            at = ((p * H + y0) * W + x0, W)
            windows.append((sg, h, w, at, [at] * len(cands)))
    flat = [t.detach().float().contiguous().reshape(-1) for t in cands]
    return pooled_rows(flat, gt.detach().float().contiguous().reshape(-1), windows, len(segments), value_max,
                       valid=_flat_valid("scores_pooled", valid, gt))


def _flat_valid(what, valid, gt):
    """A bool or uint8 validity tensor of gt's shape on gt's device -> the flat uint8 plane `pooled_rows` takes (None stays
    None)."""
    if valid is None:
        return None
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8) or valid.shape != gt.shape:
        raise ValueError(f"{what}: valid must be a bool or uint8 tensor of the ground truth's shape {tuple(gt.shape)}")
    if valid.device != gt.device:
        raise ValueError(f"{what}: valid on {valid.device}, the ground truth on {gt.device}")
    valid = valid.detach().contiguous().reshape(-1)
    return valid.view(torch.uint8) if valid.dtype == torch.bool else valid     # a bool is one byte, 0 or 1


class ScenePredictions:
    """Collects the predictions of a `data.TileCropBatches(scenes, B, patch_size, patches_per_image)` pass as metre mosaics.

    add(pred, meta): pred (B, 1, k, k) in the network's range with the batch's meta, any batch size, scenes possibly split
    across batches, in the pass's order.  Whole scenes are assembled by ONE launch per call (K12(a): clamp, de-scale,
    + base, feather merge) into one pooled device buffer; the tiles of a scene still incomplete wait for the next call.
    With `patch_size` not smaller than the scenes (the 8 m set-up, one patch per image) the raster is the de-scaled tile,
    uncropped.  All scenes must be square and of one size (one cover per launch).
    rasters(): {scene id: (h, w) float32 numpy array} with one device-to-host copy -- what the reference writes to GeoTIFF.
    `buffer` (flat fp32), `offsets` (per scene, elements) and `shape` describe the pool for `summarise`."""

    def __init__(self, scenes, patch_size: int, patches_per_image: int, border: float = 0.0):
        shapes = set(scenes.shapes)
        if len(shapes) != 1 or scenes.shapes[0][0] != scenes.shapes[0][1]:
            raise ValueError(f"ScenePredictions: square scenes of one size, got {sorted(shapes)}")
        self.scenes, self.k, self.n, self.border = scenes, int(patch_size), int(patches_per_image), float(border)
        full = scenes.shapes[0][0]
        self.full = full
        if self.k >= full:                                    # no crop (data_utils.py:108-109): one k = full tile per scene
            if self.n != 1:
                raise NotImplementedError(f"ScenePredictions: uncropped scenes with {self.n} patches per image (1 is built)")
            self.k = self.side = full
            self.n_x, self.b, self.stride = 1, 0, 0
        else:
            self.n_x = math.isqrt(self.n)
            if self.n_x * self.n_x != self.n or self.n_x not in (2, 3):
                raise NotImplementedError(f"n {self.n} is not 9 or 4")
            self.b = int(self.k * self.border)
            w_l_c = self.k - 2 * self.b
            self.side = full - 2 * self.b
            self.stride, n2 = T.get_tile(self.side, w_l_c)
            if n2 != self.n or self.stride != T.get_tile(full, self.k, self.n)[0]:
                raise ValueError(f"ScenePredictions: {self.n} tiles of {self.k} do not cover a {full}-pixel scene")
        self.shape = (self.side, self.side)
        S, dev = len(scenes), scenes.device
        self.offsets = [i * self.side * self.side for i in range(S)]
        self.buffer = torch.empty(S * self.side * self.side, dtype=torch.float32, device=dev)
        self._base = torch.tensor([float(np.float32(b)) for b in scenes.base], dtype=torch.float32, device=dev)
        self._off = torch.tensor(self.offsets, dtype=torch.int64, device=dev)
        p = self.k - 2 * self.b - self.stride if self.n_x > 1 else 0
        self._ramp = (torch.linspace(1, 0, p + 2, dtype=torch.float64)[1:-1].to(device=dev, dtype=torch.float32).contiguous()
                      if p > 0 else None)
        self.reset()

    def reset(self):
        self._pending, self._tiles = None, 0

    @property
    def complete(self) -> bool:
        return self._tiles == len(self.scenes) * self.n

    @torch.no_grad()
    def add(self, pred: torch.Tensor, meta=None):
        if pred.dim() != 4 or pred.shape[1] != 1 or pred.shape[2] != self.k or pred.shape[3] != self.k:
            raise ValueError(f"ScenePredictions.add: (B, 1, {self.k}, {self.k}) predictions, got {tuple(pred.shape)}")
        if pred.device != self.buffer.device:
            raise ValueError(f"ScenePredictions.add: predictions on {pred.device}, the scenes on {self.buffer.device}")
        B = pred.shape[0]
        if self._tiles + B > len(self.scenes) * self.n:
            raise ValueError("ScenePredictions.add: more tiles than the scenes hold")
        if meta is not None:
            if len(meta) != B:
                raise ValueError(f"ScenePredictions.add: {len(meta)} meta entries for a batch of {B}")
            for j, m in enumerate(meta):
                want = self.scenes.ids[(self._tiles + j) // self.n]
                if isinstance(m, dict) and "id" in m and str(m["id"]) != want:
                    raise ValueError(f"ScenePredictions.add: tile {self._tiles + j} belongs to scene {want}, its meta says {m['id']}")
        t = pred.detach().float()
        if self._pending is not None:
            t = torch.cat((self._pending, t))
        s0 = (self._tiles - (0 if self._pending is None else self._pending.shape[0])) // self.n
        whole = t.shape[0] // self.n
        self._tiles += B
        if whole:
            self._assemble(t[:whole * self.n].contiguous(), s0, whole)
        rest = t[whole * self.n:]
        self._pending = rest.clone() if rest.shape[0] else None

    def _assemble(self, t, s0, S):
        sc = self.scenes
        if t.is_cuda:
            _lib.check(_lib.load().jspsr_scenes_assemble_f32(
                t.data_ptr(), self._base.data_ptr() + 4 * s0, self._ramp.data_ptr() if self._ramp is not None else None,
                self.buffer.data_ptr(), self._off.data_ptr() + 8 * s0, self.buffer.numel(), S, self.n_x, self.k, self.b, self.stride,
                int(bool(sc.elev_log)), float(sc.elev_min), float(sc.elev_max), torch.cuda.current_stream(t.device).cuda_stream),
                "jspsr_scenes_assemble_f32")
            return
        for i in range(S):                                     # the composition itself, as torch operators
            m = compose_scene(t[i * self.n:(i + 1) * self.n], self._base[s0 + i], self.full, self.border, sc.elev_min, sc.elev_max,
                              sc.elev_log)
            o = self.offsets[s0 + i]
            self.buffer[o:o + m.numel()] = m.reshape(-1)

    def rasters(self) -> dict:
        if not self.complete:
            raise ValueError(f"ScenePredictions.rasters: {self._tiles} of {len(self.scenes) * self.n} tiles were added")
        host = self.buffer.cpu().numpy()
        n = self.side * self.side
        return {sid: host[o:o + n].reshape(self.shape).copy() for sid, o in zip(self.scenes.ids, self.offsets)}


def compose_scene(tiles, base, full, border, elev_min, elev_max, elev_log):
    """One scene the way the package's own steps give it: clamp -> `metrics.descale_data` -> + base -> `tiles.merge_tiles`
    (a single uncropped tile is returned de-scaled).  tiles (n, 1, k, k) in the network's range; base a number or a 0-d
    fp32 tensor.  K12(a) gives these bits for all scenes of a batch in one launch."""
    m = M.descale_data(tiles.float().clamp(0.0, 1.0), elev_min, elev_max, elev_log) + base
    if tiles.shape[0] == 1 and tiles.shape[-1] >= full:
        return m[0, 0]
    return T.merge_tiles(m, full, border)


def store_layout(scenes, rasters, name="baseline", what="summarise"):
    """A list of (h, w) metre rasters -> one flat fp32 buffer in the store's layout, uploaded once."""
    if len(rasters) != len(scenes):
        raise ValueError(f"{what}: baseline {name!r} has {len(rasters)} rasters, the store {len(scenes)} scenes")
    flat = []
    for i, r in enumerate(rasters):
        a = r.detach().cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r)
        a = a.reshape(a.shape[:2]) if a.ndim == 3 and a.shape[2] == 1 else a
        if tuple(a.shape) != tuple(scenes.shapes[i]):
            raise ValueError(f"{what}: baseline {name!r}[{i}] is {a.shape}, the scene {scenes.shapes[i]}")
        flat.append(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
    return torch.from_numpy(np.concatenate(flat)).to(scenes.device)


def _valid_layout(scenes, valid, numel, device, what="summarise"):
    """`summarise`'s valid -> the flat uint8 plane in store layout on the store's device."""
    if isinstance(valid, torch.Tensor) and valid.dim() == 1:
        if valid.numel() != numel or valid.dtype != torch.uint8 or valid.device != device:
            raise ValueError(f"{what}: a flat valid tensor must be uint8 with the store's layout and device")
        return valid.contiguous()
    if len(valid) != len(scenes):
        raise ValueError(f"{what}: valid has {len(valid)} planes, the store {len(scenes)} scenes")
    flat = []
    for i, v in enumerate(valid):
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        a = a.reshape(a.shape[:2]) if a.ndim == 3 and a.shape[2] == 1 else a
        if a.dtype not in (np.bool_, np.uint8) or tuple(a.shape) != tuple(scenes.shapes[i]):
            raise ValueError(f"{what}: valid[{i}] is {a.dtype} {a.shape}, expected a bool or uint8 plane of {tuple(scenes.shapes[i])}")
        flat.append((a.reshape(-1) != 0).astype(np.uint8))
    return torch.from_numpy(np.concatenate(flat)).to(device)


def valid_plane(scenes, nodata, also=None) -> torch.Tensor:
    """The flat uint8 plane, in store layout on the store's device, of the pixels whose ground truth can be scored:
    `hr_dem` finite and -- unless `nodata` is NaN -- != np.float32(nodata) (the complement of `data.void_pixels`), formed
    with torch operators on the device.  also: one further plane of the same layout, or a list of them (bool or uint8,
    e.g. `(inference_scenes.void_out == 0)` of a K17 store over the same scenes), ANDed in.  -> `summarise(valid=...)`."""
    gt = scenes.store["hr_dem"]
    keep = torch.isfinite(gt)
    nd = np.float32(nodata)
    if not np.isnan(nd):
        keep &= gt != float(nd)
    if also is not None:
        for p in ([also] if isinstance(also, torch.Tensor) else list(also)):
            if not isinstance(p, torch.Tensor) or p.dim() != 1 or p.numel() != gt.numel() or p.device != gt.device \
                    or p.dtype not in (torch.bool, torch.uint8):
                raise ValueError("valid_plane: `also` takes flat bool / uint8 planes with the store's layout and device")
            keep &= p != 0
    return keep.to(torch.uint8)


def _assemble(what, scenes, predictions, baselines, border, patch_size, valid):
    """What `summarise` and `error_distribution` score: the candidates' names and flat buffers ("SR" first), the ground
    truth, one border-cropped window per scene in segment 0 and the validity plane in store layout (or None)."""
    names = ["SR"] + list(baselines or {})
    if len(names) > MAX_CANDIDATES:
        raise ValueError(f"{what}: {len(names)} candidates, at most {MAX_CANDIDATES}")
    if "SR" in (baselines or {}):
        raise ValueError(f"{what}: 'SR' names the prediction")
    S = len(scenes)
    b = int(patch_size * border)
    offs = [0]
    for h, w in scenes.shapes:
        offs.append(offs[-1] + h * w)
    gt = scenes.store["hr_dem"]
    if valid is not None:
        valid = _valid_layout(scenes, valid, gt.numel(), gt.device, what)
    if isinstance(predictions, ScenePredictions):
        if predictions.scenes is not scenes or not predictions.complete:
            raise ValueError(f"{what}: the collector must be complete and made on the same scenes")
        sr, sr_off, sr_shape = predictions.buffer, predictions.offsets, [predictions.shape] * S
    else:
        if len(predictions) != S:
            raise ValueError(f"{what}: {len(predictions)} predictions for {S} scenes")
        arrs = [np.ascontiguousarray(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p, dtype=np.float32) for p in predictions]
        sr_shape = [tuple(a.shape) for a in arrs]
        sr_off = [0]
        for a in arrs:
            sr_off.append(sr_off[-1] + a.size)
        sr = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(scenes.device)
    cands = [sr]
    for name, src in (baselines or {}).items():
        if isinstance(src, str):
            if src != "lr_dem":
                raise ValueError(f"{what}: baseline {name!r}: {src!r} is not a raster of the store ('lr_dem')")
            cands.append(scenes.store["lr_dem"])
        elif isinstance(src, torch.Tensor) and src.dim() == 1:           # already in store layout, e.g. uploaded by an earlier call
            if src.numel() != gt.numel() or src.dtype != torch.float32 or src.device != gt.device:
                raise ValueError(f"{what}: baseline {name!r}: a flat tensor must have the store's layout, dtype and device")
            cands.append(src.contiguous())
        else:
            cands.append(store_layout(scenes, src, name, what))
    windows = []
    for i, (h, w) in enumerate(scenes.shapes):
        ch, cw = h - 2 * b, w - 2 * b
        if ch <= 0 or cw <= 0:
            raise ValueError(f"{what}: nothing left of scene {scenes.ids[i]} ({h} x {w}) after a crop of {b}")
        at = (offs[i] + b * w + b, w)
        if sr_shape[i] == (h, w):
            sr_at = (sr_off[i] + b * w + b, w)
        elif sr_shape[i] == (ch, cw):
            sr_at = (sr_off[i], cw)
        else:
            raise ValueError(f"{what}: prediction {scenes.ids[i]} is {sr_shape[i]}, expected {(h, w)} or {(ch, cw)}")
        windows.append((0, ch, cw, at, [sr_at] + [at] * (len(cands) - 1)))
    return names, cands, gt, windows, valid


def summarise(scenes, predictions, baselines=None, *, value_max: float, border: float = 0.0, patch_size: int, online: bool = False,
              valid=None):
    """summarise_evaluation (utils/utils.py:970-1368) on the device.

    scenes: the `data.DeviceScenes` store; the ground truth is `scenes.store["hr_dem"]`, read in place.
    predictions: a complete `ScenePredictions`, or a list of per-scene metre rasters (whole scenes or border-cropped mosaics).
    baselines: {name: "lr_dem" (the store's own input DEM) | a list of (h, w) metre rasters, one per scene, uploaded once
    in store layout (`store_layout` does it ahead of time; its flat tensor is accepted here too)}.
    Every raster loses int(patch_size * border) pixels per side (utils.py:1276-1306); a prediction that already has the
    cropped size is taken whole.  value_max: tensor_kwargs.max, PSNR's numerator.
    -> {name: {"RMSE", "Median", "NMAD", "LE95", "PSNR"}} pooled over all pixels of all scenes ("offline"), for "SR" and
    each baseline.  online=True: -> (that dict, {name: the means of the per-scene values}, {name: {scene id: the five
    values}}).  One K12(b) call, one device-to-host copy at the end, no other synchronisation.
    valid (K18): score only the pixels set in it -- a list of per-scene (h, w) bool / uint8 arrays, uploaded once in store
    layout, or a flat uint8 device tensor in store layout (`valid_plane(scenes, nodata)`; `(inference_scenes.void_out ==
    0).to(torch.uint8)` of a K17 store over the same scenes), cropped with the rasters.  One plane for all candidates: the
    rows of a table are scored over the same pixels.  Every row dict then gains "N", the number of pixels scored (a row
    without any is NaN); the means average the scenes with N > 0.  Still one call and one device-to-host copy."""
    names, cands, gt, windows, valid = _assemble("summarise", scenes, predictions, baselines, border, patch_size, valid)
    S = len(scenes)
    if online:
        windows += [(1 + i,) + wdw[1:] for i, wdw in enumerate(windows)]
    n_seg = 1 + S if online else 1
    if valid is None:
        rows = pooled_rows(cands, gt, windows, n_seg, value_max)
        host = rows.cpu().numpy().astype(np.float64)          # the one device-to-host copy
        count = None
    else:                                                     # the counts ride behind the rows: still one copy (exact below 2^53)
        rows, counts = pooled_rows(cands, gt, windows, n_seg, value_max, valid=valid)
        both = torch.cat((rows.double().reshape(-1), counts.double())).cpu().numpy()
        host = both[:rows.numel()].reshape(tuple(rows.shape))
        count = [int(v) for v in both[rows.numel():]]

    def row(c, sg):
        d = {k: float(host[c, sg, j]) for j, k in enumerate(COLUMNS)}
        if count is not None:
            d["N"] = count[sg]
        return d

    pooled = {name: row(c, 0) for c, name in enumerate(names)}
    if not online:
        return pooled
    per_scene = {name: {sid: row(c, 1 + i) for i, sid in enumerate(scenes.ids)} for c, name in enumerate(names)}
    if count is None:
        means = {name: {k: sum(v[k] for v in per_scene[name].values()) / S for k in COLUMNS} for name in names}
    else:
        means = {}
        for name in names:
            scored = [v for v in per_scene[name].values() if v["N"] > 0]
            means[name] = {k: sum(v[k] for v in scored) / len(scored) if scored else float("nan") for k in COLUMNS}
    return pooled, means, per_scene


# ---- K21: the error distribution -------------------------------------------------------------------------------------
def _f16_key(bits):
    """The order-preserving key of float16 bits (uint16 array or int): negative values reversed below the positive ones."""
    bits = np.asarray(bits, dtype=np.int64)
    return bits ^ np.where(bits & 0x8000, 0xffff, 0x8000)


def histogram_bins(lo: float = -5.0, hi: float = 5.0):
    """-> (key0, K): the key of float16(float32(lo)) and the number of float16 values from there to float16(float32(hi)),
    both included.  (-5, 5): K = 35330.  ValueError unless lo <= hi, both finite, both magnitudes <= 65504."""
    lo, hi = float(lo), float(hi)
    if not (lo <= hi and abs(lo) <= 65504.0 and abs(hi) <= 65504.0):
        raise ValueError(f"histogram_bins: lo = {lo}, hi = {hi} (lo <= hi, both finite, magnitudes <= 65504)")
    k = _f16_key(np.array([lo, hi], dtype=np.float32).astype(np.float16).view(np.uint16))
    return int(k[0]), int(k[1] - k[0] + 1)


def histogram_values(key0: int, K: int, device=None) -> torch.Tensor:
    """-> (K,) float64: the float16 value of every bin of a `pooled_histogram` (-0 and +0 are two bins of value 0)."""
    if K < 1 or key0 < 0x0400 or key0 + K - 1 > 0xfbff:
        raise ValueError(f"histogram_values: key0 = {key0}, K = {K} are not bins of finite float16 values")
    k = np.arange(key0, key0 + K, dtype=np.int64)
    bits = np.where(k & 0x8000, k ^ 0x8000, k ^ 0xffff).astype(np.uint16)
    return torch.from_numpy(bits.view(np.float16).astype(np.float64)).to(device or "cpu")


def pooled_histogram(cands: Sequence[torch.Tensor], gt: torch.Tensor, windows: Sequence[tuple], lo: float = -5.0, hi: float = 5.0,
                     valid: torch.Tensor | None = None):
    """The float16 histogram of the pooled errors (K21).  cands, gt, windows, valid: as `pooled_rows` takes them; the
    windows' segment entry is not read -- everything a call is given is one pool.  Per pooled element and candidate e =
    cand - gt in fp32; with `valid`, an element whose byte is 0 is not scored, whatever the rasters hold there.  A scored
    element with float32(lo) <= e <= float32(hi) is rounded to float16 (nearest, ties to even, subnormals kept: numpy's
    astype) and counted in bin key(e) - key0; NaN and infinities fail the comparison and poison nothing (unlike K12's rows).
    -> (hist (n_cand, K) int64, counts (n_cand, 4) int64 = {n_scored, n_in, n_below, n_above}, key0) on the buffers' device;
    n_scored - n_in - n_below - n_above is the number of NaNs.  `histogram_values(key0, K)` gives the bins' values.  Exact
    and order-free: the same bits on every run, whatever candidates share the call.  Device: one launch, no host
    synchronisation."""
    n_cand = len(cands)
    total = _check_pool("pooled_histogram", cands, gt, windows, valid)
    if not windows:
        raise ValueError("pooled_histogram: no windows")
    key0, K = histogram_bins(lo, hi)
    if total >= 2 ** 32:
        raise ValueError(f"pooled_histogram: {total} pooled elements, the bin counters hold fewer than 2^32")
    if gt.is_cuda:
        dev = gt.device
        table = _upload(_window_table(windows, False), dev)
        hist = torch.empty((n_cand, K), dtype=torch.int64, device=dev)
        counts = torch.empty((n_cand, 4), dtype=torch.int64, device=dev)
        ptrs, numel = _cand_arrays(cands)
        _lib.check(_lib.load().jspsr_errdist_hist_forward(ptrs, numel, n_cand, gt.data_ptr(), gt.numel(),
                                                          valid.data_ptr() if valid is not None else None,
                                                          valid.numel() if valid is not None else 0, table.data_ptr(), len(windows),
                                                          total, float(lo), float(hi), hist.data_ptr(), counts.data_ptr(),
                                                          torch.cuda.current_stream(dev).cuda_stream),
                   "jspsr_errdist_hist_forward")
        return hist, counts, key0
    g_np = gt.numpy()
    lo32, hi32 = np.float32(lo), np.float32(hi)
    keep = None if valid is None else np.concatenate(_gather_plane(valid.numpy(), windows)) != 0
    hist = np.zeros((n_cand, K), dtype=np.int64)
    counts = np.zeros((n_cand, 4), dtype=np.int64)
    for c, cand in enumerate(cands):
        e = np.concatenate(_gather_errors(cand.numpy(), g_np, windows, c)).astype(np.float32, copy=False)
        if keep is not None:
            e = e[keep]
        inside = (e >= lo32) & (e <= hi32)
        b = _f16_key(e[inside].astype(np.float16).view(np.uint16)) - key0
        hist[c] = np.bincount(np.clip(b, 0, K - 1), minlength=K)              # lo = +0 keeps -0: counted with +0
        counts[c] = (e.size, int(inside.sum()), int((e < lo32).sum()), int((e > hi32).sum()))
    return torch.from_numpy(hist), torch.from_numpy(counts), key0


def _kde_host(h: np.ndarray, v: np.ndarray, gridsize: int, cut: float, bw_adjust: float):
    """One candidate's curve from its counts h and the bins' values v, the formulas of include/jspsr_hip.h (K21) as numpy."""
    nan = np.full(gridsize, np.nan)
    occ = np.nonzero(h)[0]
    n = int(h.sum())
    if n < 1:
        return nan, nan, (np.nan, np.nan, np.nan)
    c, x = h[occ].astype(np.float64), v[occ]
    mean = float(np.sum(c * x) / n)
    if n < 2:
        return nan, nan, (mean, np.nan, np.nan)
    var = float(np.sum(c * (x - mean) ** 2) / (n - 1))
    sd = math.sqrt(var)
    bw = sd * float(n) ** -0.2 * bw_adjust
    if not var > 0.0:
        return nan, nan, (mean, sd, bw)
    support = np.linspace(x[0] - cut * bw, x[-1] + cut * bw, gridsize)
    dens = np.array([np.sum(c * np.exp(-(g - x) ** 2 / (2.0 * (bw * bw)))) for g in support]) / (n * bw * math.sqrt(2.0 * math.pi))
    return support, dens, (mean, sd, bw)


def kde_curves(hist: torch.Tensor, key0: int, gridsize: int = 200, cut: float = 0.5, bw_adjust: float = 1.0):
    """The Gaussian kernel density estimates seaborn's `kdeplot(bw_adjust=, cut=, gridsize=, common_norm=False)` draws, from
    `pooled_histogram`'s counts, all in fp64 (K21).  hist: (n_cand, K) or (K,) int64.  Per candidate, with c_b the counts and
    v_b the bins' values: n = sum c_b; mean = sum c_b v_b / n; var = sum c_b (v_b - mean)^2 / (n - 1); bw = sqrt(var) *
    n^(-1/5) * bw_adjust (scipy's gaussian_kde with scotts_factor and set_bandwidth(factor * bw_adjust), what seaborn 0.12+
    does); support = linspace(vmin - cut bw, vmax + cut bw, gridsize) over the occupied bins (seaborn's
    _define_support_grid with clip=None); density_j = sum c_b exp(-(g_j - v_b)^2 / (2 bw^2)) / (n bw sqrt(2 pi)).
    seaborn is not a dependency and was not available to pin against: the curve is pinned to scipy.stats.gaussian_kde and to
    the rule above (tests/errdist_ref.py), not to seaborn itself.
    -> (support (n_cand, gridsize), density (n_cand, gridsize), stats (n_cand, 3) = {mean, std, bw}), fp64 tensors on the
    histogram's device ((gridsize,), (gridsize,), (3,) for a (K,) histogram).  n < 2 or var == 0: support and density are NaN
    (seaborn draws nothing there).  Device: two launches, no host synchronisation; the same bits on every run."""
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or hist.dim() not in (1, 2):
        raise ValueError("kde_curves: an int64 (n_cand, K) or (K,) histogram")
    one = hist.dim() == 1
    h2 = (hist[None] if one else hist).contiguous()
    n_cand, K = h2.shape
    if not 1 <= n_cand <= MAX_CANDIDATES:
        raise ValueError(f"kde_curves: {n_cand} candidates, 1..{MAX_CANDIDATES} are taken")
    if K < 1 or key0 < 0x0400 or key0 + K - 1 > 0xfbff:
        raise ValueError(f"kde_curves: key0 = {key0}, K = {K} are not bins of finite float16 values")
    gridsize, cut, bw_adjust = int(gridsize), float(cut), float(bw_adjust)
    if not (2 <= gridsize <= 65535 and 0.0 <= cut < math.inf and 0.0 < bw_adjust < math.inf):
        raise ValueError(f"kde_curves: gridsize = {gridsize}, cut = {cut}, bw_adjust = {bw_adjust} (gridsize >= 2, cut >= 0, bw_adjust > 0)")
    if h2.is_cuda:
        dev = h2.device
        lib = _lib.load()
        support = torch.empty((n_cand, gridsize), dtype=torch.float64, device=dev)
        density = torch.empty((n_cand, gridsize), dtype=torch.float64, device=dev)
        stats = torch.empty((n_cand, 3), dtype=torch.float64, device=dev)
        ws = torch.empty(lib.jspsr_errdist_workspace_bytes(n_cand, gridsize), dtype=torch.uint8, device=dev)
        _lib.check(lib.jspsr_errdist_kde_forward(h2.data_ptr(), n_cand, key0, K, gridsize, cut, bw_adjust, support.data_ptr(),
                                                 density.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "jspsr_errdist_kde_forward")
    else:
        v = histogram_values(key0, K).numpy()
        got = [_kde_host(h, v, gridsize, cut, bw_adjust) for h in h2.numpy()]
        support, density, stats = (torch.from_numpy(np.array([g[i] for g in got], dtype=np.float64)) for i in range(3))
    return (support[0], density[0], stats[0]) if one else (support, density, stats)


def error_distribution(scenes, predictions, baselines=None, *, border: float = 0.0, patch_size: int, valid=None, lo: float = -5.0,
                       hi: float = 5.0, gridsize: int = 200, cut: float = 0.5, bw_adjust: float = 1.0):
    """The curves of the reference's figure "Elevation Error Distribution in [-5, 5] m" (summarise_evaluation,
    utils/utils.py:1394-1456) on the device: per candidate all pooled errors with lo <= e <= hi, as float16, under
    `sns.kdeplot(bw_adjust=1, cut=0.5, common_norm=False)`.  Drawing stays out.
    scenes, predictions, baselines, border, patch_size, valid: as `summarise` takes them, with the same crops.
    -> {name: {"support", "density" (numpy float64, (gridsize,)), "n" (pixels scored), "n_in", "n_below", "n_above", "mean",
    "std", "bw"}} for "SR" and each baseline.  `pooled_histogram` and `kde_curves` (whose docstrings state the arithmetic
    and what it is pinned to), then one device-to-host copy; no other synchronisation."""
    names, cands, gt, windows, valid = _assemble("error_distribution", scenes, predictions, baselines, border, patch_size, valid)
    hist, counts, key0 = pooled_histogram(cands, gt, windows, lo, hi, valid=valid)
    support, density, stats = kde_curves(hist, key0, gridsize, cut, bw_adjust)
    n_c, G = len(names), support.shape[1]
    both = torch.cat((support.reshape(-1), density.reshape(-1), stats.reshape(-1), counts.double().reshape(-1))).cpu().numpy()   # the one copy
    sup, den = both[:n_c * G].reshape(n_c, G), both[n_c * G:2 * n_c * G].reshape(n_c, G)
    st, cnt = both[2 * n_c * G:2 * n_c * G + 3 * n_c].reshape(n_c, 3), both[2 * n_c * G + 3 * n_c:].reshape(n_c, 4)   # counts: exact below 2^53
    return {name: {"support": sup[c].copy(), "density": den[c].copy(), "n": int(cnt[c, 0]), "n_in": int(cnt[c, 1]),
                   "n_below": int(cnt[c, 2]), "n_above": int(cnt[c, 3]), "mean": float(st[c, 0]), "std": float(st[c, 1]),
                   "bw": float(st[c, 2])} for c, name in enumerate(names)}


# ---- K22: scores by terrain class ------------------------------------------------------------------------------------
MAX_CLASSES = 32
MAX_SLOPE_EDGES = 31
NO_CLASS = 255                # the label of a pixel that belongs to no class


def _check_labels(what, labels, gt, n_classes):
    if not isinstance(n_classes, int) or isinstance(n_classes, bool) or not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"{what}: n_classes = {n_classes!r}, 1..{MAX_CLASSES} are taken")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 1 or not labels.is_contiguous():
        raise ValueError(f"{what}: labels must be a flat contiguous uint8 tensor")
    if labels.numel() != gt.numel():
        raise ValueError(f"{what}: labels has {labels.numel()} elements, the ground truth {gt.numel()}")
    if labels.device != gt.device:
        raise ValueError(f"{what}: labels on {labels.device}, the ground truth on {gt.device}")


def stratified_rows(cands: Sequence[torch.Tensor], gt: torch.Tensor, windows: Sequence[tuple], labels: torch.Tensor, n_classes: int,
                    value_max: float, valid: torch.Tensor | None = None):
    """The raw per-class table call (K22).  cands, gt, windows, valid: as `pooled_rows` takes them; the windows' segment
    entry is not read -- everything a call is given is one pool.  labels: a flat contiguous uint8 tensor of gt.numel()
    elements on gt's device, read at gt's offsets and pitches as `valid` is.  A pooled element belongs to class c =
    labels[i] iff c < n_classes (1..32) and (valid is None or valid[i] != 0); every other element (a label of 255, a label
    >= n_classes, a masked one) influences nothing, whatever the rasters hold there.
    -> (rows (n_cand, n_classes, 11) fp32, columns `ROW`; counts (n_classes,) int64) on the buffers' device.  Per class the
    row is `pooled_rows(..., valid=(labels == c) & valid)`'s: the ranks come from the class count, a class without an element
    has a NaN row and count 0, a counted NaN makes that class's five scores NaN for that candidate alone.
    Device: one call of 16 launches whatever n_classes, the candidates, the windows and the data are, every pass over the
    pool serving all classes; no host synchronisation; the same bits on every run, for every n_cand."""
    n_cand = len(cands)
    total = _check_pool("stratified_rows", cands, gt, windows, valid)
    _check_labels("stratified_rows", labels, gt, n_classes)
    if not windows:
        raise ValueError("stratified_rows: no windows")
    if total >= 2 ** 32:
        raise ValueError(f"stratified_rows: {total} pooled elements, the rank counters hold fewer than 2^32")
    if gt.is_cuda:
        lib = _lib.load()
        nbytes = lib.jspsr_strata_workspace_bytes(n_cand, n_classes, total)
        if nbytes == 0:
            raise ValueError(f"stratified_rows: {n_cand} candidates, {n_classes} classes, {total} pooled elements: not a size K22 takes")
        dev = gt.device
        table = _upload(_window_table(windows, False), dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty((n_cand, n_classes, len(ROW)), dtype=torch.float32, device=dev)
        counts = torch.empty(n_classes, dtype=torch.int64, device=dev)
        ptrs, numel = _cand_arrays(cands)
        _lib.check(lib.jspsr_strata_forward(ptrs, numel, n_cand, gt.data_ptr(), gt.numel(), labels.data_ptr(), labels.numel(), n_classes,
                                            valid.data_ptr() if valid is not None else None,
                                            valid.numel() if valid is not None else 0, table.data_ptr(), len(windows), total,
                                            float(value_max), out.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "jspsr_strata_forward")
        return out, counts
    g_np = gt.numpy()
    cls = np.concatenate(_gather_plane(labels.numpy(), windows)).astype(np.int64)
    if valid is not None:
        cls[np.concatenate(_gather_plane(valid.numpy(), windows)) == 0] = NO_CLASS
    out = np.empty((n_cand, n_classes, len(ROW)), dtype=np.float32)
    for c, cand in enumerate(cands):
        e = np.concatenate(_gather_errors(cand.numpy(), g_np, windows, c)).astype(np.float32, copy=False)
        for k in range(n_classes):
            ek = e[cls == k]
            out[c, k] = _row_host(ek, value_max) if ek.size else _nan_row()
    return torch.from_numpy(out), torch.from_numpy(np.bincount(cls[cls < n_classes], minlength=n_classes).astype(np.int64))


def scores_by_class(cands, gt, labels, n_classes: int, value_max: float = 1.0, valid=None):
    """Per-class pooled scores of equal-shape tensors, `scores_pooled`'s sibling (K22).  cands: a tensor or a list of up to 8,
    each of gt's shape (..., H, W), fp32 metres; labels: a uint8 tensor of gt's shape on gt's device; valid: a bool or uint8
    tensor of gt's shape, or None.  -> (rows (n_cand, n_classes, 11), counts (n_classes,)) as `stratified_rows` gives them."""
    cands = [cands] if isinstance(cands, torch.Tensor) else list(cands)
    if gt.dim() < 2 or any(c.shape != gt.shape for c in cands):
        raise ValueError(f"scores_by_class: equal (..., H, W) tensors, got {[tuple(c.shape) for c in cands]} / {tuple(gt.shape)}")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.shape != gt.shape:
        raise ValueError(f"scores_by_class: labels must be a uint8 tensor of the ground truth's shape {tuple(gt.shape)}")
    if labels.device != gt.device:
        raise ValueError(f"scores_by_class: labels on {labels.device}, the ground truth on {gt.device}")
    valid = _flat_valid("scores_by_class", valid, gt)
    H, W = gt.shape[-2:]
    planes = gt.numel() // (H * W) if H * W else 0
    windows = [(0, H, W, (p * H * W, W), [(p * H * W, W)] * len(cands)) for p in range(planes)]
    flat = [t.detach().float().contiguous().reshape(-1) for t in cands]
    return stratified_rows(flat, gt.detach().float().contiguous().reshape(-1), windows, labels.detach().contiguous().reshape(-1),
                           n_classes, value_max, valid=valid)


def slope_thresholds(edges_deg, cell: float) -> np.ndarray:
    """The thresholds `slope_class_plane` compares p = gx^2 + gy^2 of the unnormalised 3 x 3 Sobel taps with: a slope of
    `edge` degrees on a grid of `cell` metres is a rise over run of tan(edge), and the Sobel sums are 8 * cell times the
    gradient, so t_k = float32((8 * cell * tan(edge_k * pi / 180))^2), evaluated in double and rounded once.  The one place
    they are formed.  edges_deg: strictly increasing within [0, 90), at most 31; cell > 0; ValueError otherwise."""
    edges = [float(e) for e in edges_deg]
    cell = float(cell)
    if len(edges) > MAX_SLOPE_EDGES:
        raise ValueError(f"slope_thresholds: {len(edges)} edges, at most {MAX_SLOPE_EDGES} are taken")
    if any(not 0.0 <= e < 90.0 for e in edges) or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"slope_thresholds: edges_deg = {edges} must be strictly increasing within [0, 90)")
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"slope_thresholds: cell = {cell} must be positive")
    return np.array([(8.0 * cell * math.tan(e * math.pi / 180.0)) ** 2 for e in edges], dtype=np.float64).astype(np.float32)


def _slope_labels_host(z: np.ndarray, thr: np.ndarray, valid) -> np.ndarray:
    """One scene's labels as numpy float32 operators, in the kernel's operation order."""
    t = np.pad(z.astype(np.float32, copy=False), 1, mode="edge")
    h, w = z.shape
    a, b, c = t[0:h, 0:w], t[0:h, 1:w + 1], t[0:h, 2:w + 2]
    d, f = t[1:h + 1, 0:w], t[1:h + 1, 2:w + 2]
    g, hh, i = t[2:h + 2, 0:w], t[2:h + 2, 1:w + 1], t[2:h + 2, 2:w + 2]
    two = np.float32(2.0)
    with np.errstate(all="ignore"):
        gx = ((c + two * f) + i) - ((a + two * d) + g)
        gy = ((g + two * hh) + i) - ((a + two * b) + c)
        p = gx * gx + gy * gy
        lab = (thr[:, None, None] <= p[None]).sum(axis=0).astype(np.uint8) if thr.size else np.zeros((h, w), np.uint8)
    lab[np.isnan(p)] = NO_CLASS
    if valid is not None:
        v = np.pad(valid != 0, 1, mode="edge")
        ok = np.ones((h, w), bool)
        for dy in range(3):
            for dx in range(3):
                ok &= v[dy:dy + h, dx:dx + w]
        lab[~ok] = NO_CLASS
    return lab


def slope_class_plane(scenes, edges_deg, cell: float, source: str = "hr_dem", valid=None) -> torch.Tensor:
    """A slope-class label plane for `summarise_by_class`: flat uint8, in store layout on the store's device (K22, one launch).
    Per pixel of `scenes.store[source]` ("hr_dem" or "lr_dem", metres): the 3 x 3 taps a b c / d e f / g h i, replicate-clamped
    inside their own scene; in fp32, every operation rounded once, gx = ((c + 2f) + i) - ((a + 2d) + g), gy = ((g + 2h) + i) -
    ((a + 2b) + c), p = gx*gx + gy*gy; label = the number of `slope_thresholds(edges_deg, cell)` that are <= p, so class k
    holds the slopes in [edge_{k-1}, edge_k) and len(edges_deg) + 1 classes come out.  255 where p is NaN or, with `valid`
    (a flat uint8 plane in store layout, or a list of per-scene planes), where any of the nine clamped taps is invalid.
    cell: the grid spacing in metres.  ValueError for bad edges or cell before any launch."""
    thr = slope_thresholds(edges_deg, cell)
    if source not in ("hr_dem", "lr_dem"):
        raise ValueError(f"slope_class_plane: source {source!r} is not a metre raster of the store ('hr_dem', 'lr_dem')")
    z = scenes.store[source]
    numel = sum(h * w for h, w in scenes.shapes)
    if valid is not None:
        valid = _valid_layout(scenes, valid, numel, z.device, "slope_class_plane")
    if z.is_cuda:
        out = torch.empty(numel, dtype=torch.uint8, device=z.device)
        t = (ctypes.c_float * max(len(thr), 1))(*[float(v) for v in thr])
        _lib.check(_lib.load().jspsr_slope_classes(z.data_ptr(), numel, scenes.scene_table.data_ptr(), len(scenes), t, len(thr),
                                                   valid.data_ptr() if valid is not None else None,
                                                   valid.numel() if valid is not None else 0, out.data_ptr(),
                                                   torch.cuda.current_stream(z.device).cuda_stream), "jspsr_slope_classes")
        return out
    z_np, v_np, off, flat = z.numpy(), None if valid is None else valid.numpy(), 0, []
    for h, w in scenes.shapes:
        flat.append(_slope_labels_host(z_np[off:off + h * w].reshape(h, w), thr,
                                       None if v_np is None else v_np[off:off + h * w].reshape(h, w)).reshape(-1))
        off += h * w
    return torch.from_numpy(np.concatenate(flat))


def _labels_layout(scenes, labels, numel, device, what):
    """`summarise_by_class`'s labels -> the flat uint8 plane in store layout on the store's device."""
    if isinstance(labels, torch.Tensor) and labels.dim() == 1:
        if labels.numel() != numel or labels.dtype != torch.uint8 or labels.device != device:
            raise ValueError(f"{what}: a flat labels tensor must be uint8 with the store's layout ({numel} elements) and device")
        return labels.contiguous()
    if len(labels) != len(scenes):
        raise ValueError(f"{what}: labels has {len(labels)} planes, the store {len(scenes)} scenes")
    flat = []
    for i, v in enumerate(labels):
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        a = a.reshape(a.shape[:2]) if a.ndim == 3 and a.shape[2] == 1 else a
        if a.dtype != np.uint8 or tuple(a.shape) != tuple(scenes.shapes[i]):
            raise ValueError(f"{what}: labels[{i}] is {a.dtype} {a.shape}, expected a uint8 plane of {tuple(scenes.shapes[i])}")
        flat.append(np.ascontiguousarray(a).reshape(-1))
    return torch.from_numpy(np.concatenate(flat)).to(device)


def summarise_by_class(scenes, predictions, labels, class_names, baselines=None, *, value_max: float, border: float = 0.0,
                       patch_size: int, valid=None):
    """`summarise`'s pooled table broken down by terrain class (K22).

    scenes, predictions, baselines, value_max, border, patch_size, valid: as `summarise` takes them -- the candidates, the
    windows and the crop are exactly its own.  labels: a flat uint8 device plane in store layout (`slope_class_plane`, or
    made from the store's land-cover mask, see below), or a list of per-scene (h, w) uint8 arrays, uploaded once; class c
    is named class_names[c], n_classes = len(class_names) (1..32); a label >= n_classes (255 by convention) belongs to no
    class.  One plane for all candidates.
    -> {candidate: {class name: {"RMSE", "Median", "NMAD", "LE95", "PSNR", "N", "share"}}}: N the pixels scored, share = N /
    the sum of N over the classes (NaN when no pixel has a class); a class without a pixel has NaN scores.
    One K22 call and one device-to-host copy (the counts ride behind the rows), no other synchronisation.

    Land-cover labels from a store's one-hot mask with torch operators (the first set channel, else 255; not hot):

        m = scenes.store["mask"].view(-1, C)                     # (pixels, C) uint8, store layout
        on = m.ne(0)
        labels = torch.where(on.any(1), on.to(torch.uint8).argmax(1), 255).to(torch.uint8)
    """
    class_names = [str(n) for n in class_names]
    if not 1 <= len(class_names) <= MAX_CLASSES or len(set(class_names)) != len(class_names):
        raise ValueError(f"summarise_by_class: {len(class_names)} class names, 1..{MAX_CLASSES} distinct ones are taken")
    names, cands, gt, windows, valid = _assemble("summarise_by_class", scenes, predictions, baselines, border, patch_size, valid)
    labels = _labels_layout(scenes, labels, gt.numel(), gt.device, "summarise_by_class")
    n_classes = len(class_names)
    rows, counts = stratified_rows(cands, gt, windows, labels, n_classes, value_max, valid=valid)
    both = torch.cat((rows.double().reshape(-1), counts.double())).cpu().numpy()      # the one copy (counts: exact below 2^53)
    host = both[:rows.numel()].reshape(tuple(rows.shape))
    count = [int(v) for v in both[rows.numel():]]
    n_all = sum(count)
    table = {}
    for c, name in enumerate(names):
        table[name] = {}
        for k, cname in enumerate(class_names):
            d = {col: float(host[c, k, j]) for j, col in enumerate(COLUMNS)}
            d["N"] = count[k]
            d["share"] = count[k] / n_all if n_all else float("nan")
            table[name][cname] = d
    return table
