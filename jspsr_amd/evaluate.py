"""The validation pass of the reference's training loop on the device: `PerformanceMeter`, `evaluate` (eval_model
without plotting and disk output), `validate_results`, `do_eval`.

Restates evaluation/evaluate_utils.py: PerformanceMeter :26-47, get_meter :50-118, validate_results :121-151, do_eval
:211-239, eval_model :274-357, and the per-sample record of MeterRMSE (evaluation/metrics.py:404-420).  The reference
runs the model and one meter object per score on ONE tile per step (valid_batch_size 1) and reads every value back with
`.item()`; here a batch of any size is scored by one launch (`metrics.batch_scores`, K10), the rows stay in a device
table, and a pass ends in one device-to-host copy.

Left out: plotting, GeoTIFF output and the skimage and richdem packages.
(EarlyStopper is in jspsr_amd/train.py; the scene mosaics and summarise_evaluation's table in jspsr_amd/summary.py, fed
through `evaluate(..., collector=)`.)
"""
from __future__ import annotations

from math import exp

import numpy as np
import torch
import torch.nn.functional as F

from . import metrics as M
from .data import batch_pair

# get_meter's names (case-insensitive) -> package -> column of metrics.batch_scores, or the SSIM package
_COLUMN = {
    "psnr": {"piq": 0, "local": 1},
    "rmse": {"local": 2},
    "median": {"local": 3},
    "nmad": {"local": 4},
    "le95": {"local": 5},
    "slope": {"local": 6, "kornia": 7},
    "ssim": {"piq": "piq", "local": "local"},
}


def _sobel_pair(dtype):
    gx = torch.tensor([[2.0, 0.0, -2.0], [4.0, 0.0, -4.0], [2.0, 0.0, -2.0]], dtype=dtype)
    gy = torch.tensor([[2.0, 4.0, 2.0], [0.0, 0.0, 0.0], [-2.0, -4.0, -2.0]], dtype=dtype)
    return torch.stack((gx, gy)).unsqueeze(1)


def _ssim_torch(p, g, package, valid=None):
    """metrics.ssim's two forms as torch operators (CPU tensors): "piq" valid 11x11 Gaussian (sigma 1.5), "local" the
    reference's own window (metrics.local_window) with zero padding 5.
    valid: a bool plane of p's shape -> (per-tile values (B,) fp32, counts (B,) int32) under the window rule of
    `metrics.ssim_tiles`: p and g are zeroed at the invalid pixels, a map element counts iff an 11x11 box filter of the
    invalid plane (the same padding: a padded tap is not a void) is 0 there, the mean is over the counted elements of each
    tile and over its channels; NaN where the count is 0."""
    if package == "local":
        w, pad = M.local_window(), 5
    else:
        w = torch.tensor([exp(-((x - 5) ** 2) / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
        w, pad = w / w.sum(), 0
    C = p.shape[1]
    win = torch.outer(w, w).to(p.dtype).view(1, 1, 11, 11).expand(C, 1, 11, 11)

    def filt(t):
        return F.conv2d(t, win, padding=pad, groups=C)

    if valid is not None:
        zero = torch.zeros_like(p)
        p, g = torch.where(valid, p, zero), torch.where(valid, g, zero)
    mx, my = filt(p), filt(g)
    sxx, syy, sxy = filt(p * p) - mx * mx, filt(g * g) - my * my, filt(p * g) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    if valid is None:
        return smap.mean()
    counted = F.conv2d((~valid).to(p.dtype), torch.ones(C, 1, 11, 11, dtype=p.dtype), padding=pad, groups=C) == 0
    n = counted.sum((1, 2, 3))
    total = torch.where(counted, smap, torch.zeros_like(smap)).sum((1, 2, 3))
    return torch.where(n > 0, total / n.clamp_min(1), torch.full_like(total, float("nan"))).float(), n.to(torch.int32)


def _masked_row(p, g, v, vmin, vmax, elev_log, sob):
    """One tile of `_scores_torch(valid=)`: p, g the prepared (1,1,h,w) pair, v the cropped (1,1,h,w) bool plane ->
    ((8,) fp32, [N, N_sl, N_sk]).  pred and gt are zeroed at the masked pixels first (they have no influence by
    definition, and a NaN there would poison the convolutions' products); a counted Sobel output reads valid taps only."""
    zero = torch.zeros_like(p)
    p, g = torch.where(v, p, zero), torch.where(v, g, zero)
    P, G = M.descale_data(p, vmin, vmax, elev_log), M.descale_data(g, vmin, vmax, elev_log)
    P, G = torch.where(v, P, zero), torch.where(v, G, zero)
    vf = v.float()
    c_sl = -F.max_pool2d(-vf, 3, stride=1) == 1                                          # nine taps valid, interior positions
    c_sk = -F.max_pool2d(-F.pad(vf, (1, 1, 1, 1), mode="replicate"), 3, stride=1) == 1   # nine clamped taps valid
    n, n_sl, n_sk = int(v.sum()), int(c_sl.sum()), int(c_sk.sum())
    nan = torch.tensor(float("nan"))
    row = [nan] * 8
    if n:
        dh = (P - G)[v]
        mse = ((p - g)[v] ** 2).mean()
        row[0] = -10.0 * torch.log10(mse + 1e-8)
        row[1] = 20.0 * torch.log10(1.0 / torch.sqrt(mse)) if mse.item() != 0 else torch.tensor(100.0)
        row[2:6] = M.rmse(dh), M.median(dh), M.nmad(dh), M.le95(dh)
    if n_sl:
        slope = F.conv2d(P, sob).pow(2).sum(1, keepdim=True).sqrt() - F.conv2d(G, sob).pow(2).sum(1, keepdim=True).sqrt()
        row[6] = (slope[c_sl].pow(2).sum() / n_sl).sqrt()
    if n_sk:
        grad = F.conv2d(F.pad(P - G, (1, 1, 1, 1), mode="replicate"), sob) / 16.0
        row[7] = (grad.pow(2).sum(1, keepdim=True)[c_sk].sum() / (2 * n_sk)).sqrt()
    return torch.stack([r.float().reshape(()) for r in row]), [n, n_sl, n_sk]


def _scores_torch(pred, gt, vmin, vmax, border, elev_log, valid=None):
    """metrics.batch_scores as torch operators, for CPU tensors: (B,1,H,W) -> (B, 8) fp32; with a (B,1,H,W) bool / uint8
    plane `valid` -> ((B, 8) fp32, (B, 3) int32 counts), the rules of the masked kernel (K20)."""
    rows = []
    sob = _sobel_pair(torch.float32)
    if valid is not None:
        if not torch.is_tensor(valid) or valid.shape != pred.shape or valid.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"_scores_torch: valid must be a {tuple(pred.shape)} bool / uint8 plane")
        H, W = pred.shape[-2:]
        bh, bw = int(H * border), int(W * border)
        counts = []
        for i in range(pred.shape[0]):
            p, g = M.prepare(pred[i:i + 1].float(), gt[i:i + 1].float(), border)
            row, cnt = _masked_row(p, g, valid[i:i + 1, :, bh:H - bh, bw:W - bw] != 0, vmin, vmax, elev_log, sob)
            rows.append(row)
            counts.append(cnt)
        return torch.stack(rows), torch.tensor(counts, dtype=torch.int32).reshape(-1, 3)
    for i in range(pred.shape[0]):
        p, g = M.prepare(pred[i:i + 1].float(), gt[i:i + 1].float(), border)
        P, G = M.descale_data(p, vmin, vmax, elev_log), M.descale_data(g, vmin, vmax, elev_log)
        dh = P - G
        mse = ((p - g) ** 2).mean()
        local = 20.0 * torch.log10(1.0 / torch.sqrt(mse)) if mse.item() != 0 else torch.tensor(100.0)
        slope = F.conv2d(P, sob).pow(2).sum(1).sqrt() - F.conv2d(G, sob).pow(2).sum(1).sqrt()
        q = F.pad(dh, (1, 1, 1, 1), mode="replicate")
        grad = F.conv2d(q, sob) / 16.0        # `sob` is twice the Sobel pair; Sobel / 8; the signs drop out of the squares
        rows.append(torch.stack((-10.0 * torch.log10(mse + 1e-8), local, M.rmse(dh), M.median(dh), M.nmad(dh), M.le95(dh),
                                 slope.pow(2).mean().sqrt(), grad.pow(2).mean().sqrt())))
    return torch.stack(rows)


class PerformanceMeter:
    """PerformanceMeter(p.metric) of the reference for batches of any size.

    metric_config: the reference's `metric:` mapping, e.g. {"PSNR": {"package": "piq"}, "RMSE": {"package": "local"}}
    (names case-insensitive; a missing package is "local", as get_meter defaults it).  Accepted: PSNR piq | local; RMSE,
    Median, NMAD, LE95 local; SSIM piq | local; Slope local | kornia (the kornia form is restated from kornia's public
    source and not pinned against it).  Anything else raises NotImplementedError naming the metric and the package.
    One crop and one scaling per meter: a metric entry whose own border / min / max differs from the meter's is refused.

    update() writes the batch's rows into a device table and returns without a host synchronisation: GPU batches go
    through `metrics.batch_scores` (one launch for all scores of all tiles), CPU tensors through the same formulas as
    torch operators.  SSIM is not part of that kernel: `metrics.ssim` gives a batch mean, so it is called once per sample.
    get_score() copies the table to the host once and averages in Python floats, as the reference adds `.item()` values.

    masked=True (K20): update() accepts `valid`, a (B,1,H,W) bool / uint8 plane on pred's device; the tile's scores are
    then taken over its valid pixels (`metrics.batch_scores(valid=)`; valid=None scores every pixel, with the full counts).
    The meter keeps each tile's counts {N, N_sl, N_sk} (`metrics.COUNT_COLUMNS`) beside its row -- `counts()` -- and they
    ride in the same single copy as the rows, bit for bit (int32 viewed as fp32, not converted).  A column whose count is 0
    is NaN; get_score() averages each metric over the tiles whose count FOR THAT COLUMN is positive (as summary's online
    means average the scenes with N > 0) and raises ValueError naming a metric no tile has; worst() skips NaN rows.
    An SSIM entry in a masked meter raises NotImplementedError here unless ssim_valid="window" is given (K23; without
    masked=True, or with another value, a ValueError): the SSIM column then comes from ONE `metrics.ssim_tiles` call per
    SSIM entry for the whole batch (CPU tensors: `_ssim_torch(valid=)`), over the map elements whose 11x11 window holds no
    void; counts() gains one column per SSIM entry after the three of `metrics.COUNT_COLUMNS` -- `count_names` names them
    all -- in the same single copy, and get_score() averages SSIM over the tiles whose SSIM count is positive.  An
    unmasked meter refuses `valid=` and keeps its per-sample SSIM calls."""

    def __init__(self, metric_config, value_min, value_max, border=0.05, elev_log=True, masked=False, ssim_valid=None):
        if ssim_valid is not None and ssim_valid != "window":
            raise ValueError(f"PerformanceMeter: ssim_valid must be None or 'window', got {ssim_valid!r}")
        if ssim_valid is not None and not masked:
            raise ValueError("PerformanceMeter: ssim_valid needs masked=True (an unmasked meter takes no validity plane)")
        self.config = {k: dict(v or {}) for k, v in dict(metric_config).items()}
        if not self.config:
            raise ValueError("PerformanceMeter: empty metric config")
        self.vmin, self.vmax, self.border, self.elev_log = float(value_min), float(value_max), float(border), bool(elev_log)
        self.names, self.columns = [], []
        for name, kw in self.config.items():
            package = kw.get("package") if kw.get("package") is not None else "local"
            col = _COLUMN.get(str(name).lower(), {}).get(str(package).lower())
            if col is None:
                raise NotImplementedError(f"PerformanceMeter: metric {name!r} with package {package!r} is not built")
            for key, mine in (("border", self.border), ("min", self.vmin), ("max", self.vmax)):
                if kw.get(key) is not None and float(kw[key]) != mine:
                    raise NotImplementedError(f"PerformanceMeter: metric {name!r} asks for {key} = {kw[key]}, the meter has {mine}")
            if masked and isinstance(col, str) and ssim_valid is None:
                raise NotImplementedError(f"PerformanceMeter: metric {name!r} in a masked meter: masked SSIM is not built")
            self.names.append(name)
            self.columns.append(col)
        self.masked = bool(masked)
        self.ssim_valid = ssim_valid
        # the count column each metric divides by: one of metrics.COUNT_COLUMNS, or the SSIM entry's own, appended after them
        self.count_names = list(M.COUNT_COLUMNS)
        self._count_col = []
        for name, col in zip(self.names, self.columns):
            if isinstance(col, str):
                self._count_col.append(len(self.count_names))
                self.count_names.append(f"N_{name}")
            else:
                self._count_col.append(M.COUNT_OF_COLUMN[col])
        self.reset()

    def clone(self):
        """A fresh meter with the same configuration (the reference builds a second one for the input's score)."""
        return PerformanceMeter(self.config, self.vmin, self.vmax, self.border, self.elev_log, masked=self.masked,
                                ssim_valid=self.ssim_valid)

    def reset(self):
        self._rows, self._meta, self._host = [], [], None
        self._counts, self._host_counts = [], None

    def __len__(self):
        return len(self._meta)

    @torch.no_grad()
    def update(self, pred, gt, meta=None, valid=None):
        if pred.shape != gt.shape or pred.dim() != 4 or pred.shape[1] != 1:
            raise ValueError(f"PerformanceMeter.update: equal (B,1,H,W) tensors, got {tuple(pred.shape)} {tuple(gt.shape)}")
        B = pred.shape[0]
        if meta is not None and len(meta) != B:
            raise ValueError(f"PerformanceMeter.update: {len(meta)} meta entries for a batch of {B}")
        if valid is not None and not self.masked:
            raise ValueError("PerformanceMeter.update: valid= given to a meter that was not built with masked=True")
        if self.masked:
            if valid is None:
                valid = torch.ones(pred.shape, dtype=torch.uint8, device=pred.device)
            elif not torch.is_tensor(valid) or valid.shape != pred.shape or valid.dtype not in (torch.bool, torch.uint8) or \
                    valid.device != pred.device:
                raise ValueError(f"PerformanceMeter.update: valid must be a {tuple(pred.shape)} bool / uint8 plane on {pred.device}")
            score = M.batch_scores if pred.is_cuda else _scores_torch
            full, counts = score(pred, gt, self.vmin, self.vmax, self.border, self.elev_log, valid=valid)
            cols, extra = [], []
            for c in self.columns:
                if isinstance(c, str):        # SSIM (ssim_valid="window"): every tile of the batch from one call
                    if pred.is_cuda:
                        vals, cnt = M.ssim_tiles(pred, gt, c, self.border, valid=valid)
                    else:
                        H, W = pred.shape[-2:]
                        bh, bw = int(H * self.border), int(W * self.border)
                        pp, gg = M.prepare(pred.float(), gt.float(), self.border)
                        vals, cnt = _ssim_torch(pp, gg, c, valid=valid[..., bh:H - bh, bw:W - bw] != 0)
                    cols.append(vals)
                    extra.append(cnt)
                else:
                    cols.append(full[:, c])
            self._rows.append(torch.stack(cols, dim=1))
            self._counts.append(torch.cat([counts] + [e.reshape(-1, 1) for e in extra], dim=1) if extra else counts)
            self._meta.extend(meta if meta is not None else [None] * B)
            self._host = self._host_counts = None
            return
        if all(isinstance(c, str) for c in self.columns):
            full = None
        elif pred.is_cuda:
            full = M.batch_scores(pred, gt, self.vmin, self.vmax, self.border, self.elev_log)
        else:
            full = _scores_torch(pred, gt, self.vmin, self.vmax, self.border, self.elev_log)
        cols, prepared = [], None
        for c in self.columns:
            if isinstance(c, str):            # SSIM: a batch mean per call, so one call per sample
                if prepared is None:
                    prepared = M.prepare(pred.float(), gt.float(), self.border)
                one = M.ssim if pred.is_cuda else _ssim_torch
                cols.append(torch.stack([one(prepared[0][i:i + 1], prepared[1][i:i + 1], c).float() for i in range(B)]))
            else:
                cols.append(full[:, c])
        rows = torch.stack(cols, dim=1)
        self._rows.append(rows)
        self._meta.extend(meta if meta is not None else [None] * B)
        self._host = None

    def _device_table(self):
        """(N, n_metrics) on the device the rows were made on; no host synchronisation."""
        if not self._rows:
            return torch.empty((0, len(self.columns)), dtype=torch.float32)
        if len(self._rows) > 1:
            self._rows = [torch.cat(self._rows)]
        return self._rows[0]

    def _device_counts(self):
        """(N, len(count_names)) int32 on the device the rows were made on (masked meters); no host synchronisation."""
        if not self._counts:
            return torch.empty((0, len(self.count_names)), dtype=torch.int32)
        if len(self._counts) > 1:
            self._counts = [torch.cat(self._counts)]
        return self._counts[0]

    def _fetch_own(self):
        if self._host is None or (self.masked and self._host_counts is None):
            _fetch([self], None)

    def counts(self):
        """(N_tiles, len(count_names)) int32 numpy array of a masked meter, columns `count_names`: the three of
        `metrics.COUNT_COLUMNS`, then one per SSIM entry (ssim_valid="window"); the same single copy as the table's."""
        if not self.masked:
            raise ValueError("PerformanceMeter.counts: the meter was not built with masked=True")
        self._fetch_own()
        return self._host_counts

    def table(self):
        """-> ((N, n_metrics) float32 numpy array in config order, the list of meta entries): ONE device-to-host copy,
        kept until the next update."""
        if self.masked:
            self._fetch_own()
        elif self._host is None:
            self._host = self._device_table().cpu().numpy()
        return self._host, list(self._meta)

    def get_score(self):
        """{name: average over the samples} in config order."""
        t, _ = self.table()
        if t.shape[0] == 0:
            raise ValueError("PerformanceMeter.get_score: no sample scored")
        if not self.masked:
            return {name: sum(float(v) for v in t[:, j]) / t.shape[0] for j, name in enumerate(self.names)}
        counts, out = self.counts(), {}
        for j, name in enumerate(self.names):
            keep = counts[:, self._count_col[j]] > 0
            if not keep.any():
                raise ValueError(f"PerformanceMeter.get_score: no tile has a valid pixel for metric {name!r}")
            out[name] = sum(float(v) for v in t[keep, j]) / int(keep.sum())
        return out

    def worst(self, name="RMSE", n=3):
        """MeterRMSE.get_score's "worst three" (metrics.py:404-420): the n largest values of metric `name` as
        [(meta["id"] (the sample's index where no meta was given), value)], the first occurrence on ties (np.argmax);
        empty unless more than 3 samples were scored."""
        t, meta = self.table()
        lower = [str(k).lower() for k in self.names]
        if str(name).lower() not in lower:
            raise KeyError(f"PerformanceMeter.worst: {name!r} is not among {self.names}")
        vals = [float(v) for v in t[:, lower.index(str(name).lower())]]
        ids = [m["id"] if isinstance(m, dict) and "id" in m else i for i, m in enumerate(meta)]
        if self.masked:                   # a tile without a valid pixel for this metric has no value to rank
            keep = [v == v for v in vals]
            vals, ids = [v for v, k in zip(vals, keep) if k], [i for i, k in zip(ids, keep) if k]
        out = []
        if len(vals) > 3:
            for _ in range(min(n, len(vals))):
                j = int(np.argmax(vals))
                out.append((ids[j], vals[j]))
                vals.pop(j)
                ids.pop(j)
        return out


def _fetch(meters, extra):
    """One device-to-host copy for everything a pass produced: the meters' tables (left in their caches) and `extra`
    (a 2-D device tensor or None) -> extra as a numpy array."""
    tabs = [m._device_table() for m in meters]
    cnts = [m._device_counts() if m.masked else None for m in meters]          # int32 bits behind the rows: exact
    parts = [t.reshape(-1) for t in tabs] + [c.reshape(-1).view(torch.float32) for c in cnts if c is not None] + \
            ([extra.reshape(-1).float()] if extra is not None else [])
    dev = {p.device for p in parts if p.numel()}
    if len(dev) > 1:
        raise ValueError(f"evaluate: results on several devices {sorted(map(str, dev))}")
    target = dev.pop() if dev else torch.device("cpu")
    flat = torch.cat([p.to(target) for p in parts]).cpu().numpy()
    off = 0
    for m, t in zip(meters, tabs):
        m._host = flat[off:off + t.numel()].reshape(tuple(t.shape)).copy()
        off += t.numel()
    for m, c in zip(meters, cnts):
        if c is not None:
            m._host_counts = flat[off:off + c.numel()].copy().view(np.int32).reshape(tuple(c.shape))
            off += c.numel()
    return flat[off:].reshape(tuple(extra.shape)).copy() if extra is not None else None


def _sample_additive(criterion):
    """True if every value the criterion returns for a batch is the mean of its values on the single samples."""
    spec = getattr(criterion, "spec", None)
    if spec is not None and hasattr(spec, "slots"):
        return 3 not in spec.slots                # slot 3 of losses._SLOT: BerHu
    from .losses import MultiLoss
    return isinstance(criterion, MultiLoss)       # L1 + L2 + Grad


@torch.no_grad()
def evaluate(model, batches, criterion, meter, model_name, input_data, compare_input=False, collector=None, resize_input=None):
    """eval_model (evaluate_utils.py:274-357) without plotting and disk output: `model.eval()`, no gradients, and for each
    batch of `batches` (e.g. `data.TileCropBatches`, any batch size): `criterion.reset()`, `data.batch_pair`, the
    forward, the criterion, `meter.update`.  `meter` is reset first (the reference builds a new one per call).

    -> (scores, mean Total loss, {term: mean}); with compare_input=True a fourth item, the scores of the input DEM
    `inputs[0][:, 0:1]` against the target from a second meter (evaluate_utils.py:325-342).  An input of another size
    raises NotImplementedError unless resize_input="bicubic" is given: it is then resized to the target's size on the
    device (`resample.resize`, K25: the reference's `F.interpolate(..., mode="bicubic")`, evaluate_utils.py:331-332), without
    a clamp -- the meter clamps, as in the reference.

    The loss means are weighted per sample, as `AverageMeter.update(v.item(), gt.size(0))` weights them.  With the
    reference's batch of one, every logged value is a single sample's value; to report the same means at any batch size,
    a term's batch value must be the mean of its per-sample values.  That holds for every term whose value is a plain mean
    over the elements of equally sized samples of a per-pixel quantity that reads one sample only: L1 (|d|), L2 / MSE
    (d^2), Edge / Grad (|Sobel d|, a per-plane stencil), Vanilla / BCE (a pointwise expression), Norm (1 - cosine of the
    per-pixel channel vectors) and SSIM (1 - the mean of per-plane SSIM maps).  It does NOT hold for BerHu: its threshold
    th = 0.6 * max|pred - gt| is a maximum over the WHOLE batch, and both the choice of branch and (d^2 + th^2) / (2 th)
    depend on it.  A criterion that holds BerHu is therefore fed one sample at a time (all its terms, so that Total stays
    the weighted sum of what is reported); so is a criterion of a type this module does not know.

    Loss values and scores stay on the device until the end: the pass synchronises once (one device-to-host copy).

    collector: e.g. a `summary.ScenePredictions`; its `add(pred, meta)` is called after each forward (the scene mosaics in
    metres for `summary.summarise`, the whole-set table of summarise_evaluation).  None (the default) changes nothing.

    Batches that carry "valid" (a store built with `hr_nodata` / `valid`, K19): the criterion is fed ONE SAMPLE AT A TIME
    with its slice of the plane, each sample weighing 1 as in the reference's batch of one -- a masked batch value is not
    the mean of its samples' values, because their counts of valid pixels differ.  A meter built with masked=True (K20) is
    given the plane too, and so is the input's meter under compare_input: both are scored over the same pixels, each metric
    averaged over the tiles that have a valid pixel for it, and `meter.counts()` holds every tile's counts.  A meter that
    was not built with masked=True together with such a batch raises NotImplementedError before the forward."""
    model.eval()
    if resize_input not in (None, "bicubic"):
        raise ValueError(f"evaluate: resize_input is None or 'bicubic', got {resize_input!r}")
    if meter is None and compare_input:
        raise ValueError("evaluate: compare_input needs a meter")
    if meter is not None:
        meter.reset()
    meter_in = meter.clone() if compare_input else None
    additive = _sample_additive(criterion)
    keys, rows, weights = None, [], []
    for batch in batches:
        criterion.reset()
        inputs, gt, _base, meta = batch_pair(batch, model_name, input_data)
        valid = batch.get("valid")
        if valid is not None and meter is not None and not getattr(meter, "masked", False):
            raise NotImplementedError("evaluate: a batch with a validity plane needs a meter built with masked=True "
                                      "(PerformanceMeter(..., masked=True)); this meter scores every pixel")
        pred = model(*inputs)
        if collector is not None:
            collector.add(pred, meta)
        B = gt.size(0)
        spans = [(0, B)] if additive and valid is None else [(i, i + 1) for i in range(B)]
        for lo, hi in spans:
            if lo > 0:
                criterion.reset()
            if valid is None:
                out = criterion(pred[lo:hi], gt[lo:hi])
            else:
                out = criterion(pred[lo:hi], gt[lo:hi], valid=valid[lo:hi])
            if keys is None:
                keys = list(out)
            rows.append(torch.stack([out[k].detach().float().reshape(()) for k in keys]))
            weights.append(hi - lo)
        if meter is not None:
            if valid is not None:
                meter.update(pred, gt, meta=meta, valid=valid)
            else:
                meter.update(pred, gt, meta=meta)
        if compare_input:
            data_input = inputs[0][:, 0:1]
            if data_input.shape[-2:] != gt.shape[-2:]:
                if resize_input is None:
                    raise NotImplementedError(f"evaluate: the input DEM is {tuple(data_input.shape[-2:])}, the target "
                                              f"{tuple(gt.shape[-2:])}; the reference's bicubic resize is not built")
                from .resample import resize
                data_input = resize(data_input.float(), gt.shape[-2:], resize_input)
            if valid is not None:
                meter_in.update(data_input, gt, meta=meta, valid=valid)
            else:
                meter_in.update(data_input, gt, meta=meta)
    if keys is None:
        raise ValueError("evaluate: no batches")
    vals = _fetch(([meter] if meter is not None else []) + ([meter_in] if compare_input else []),
                  torch.stack(rows)).astype(np.float64)
    total_w = sum(weights)
    means = {k: sum(float(vals[i, j]) * weights[i] for i in range(len(weights))) / total_w for j, k in enumerate(keys)}
    result = (meter.get_score() if meter is not None else None, means["Total"], {k: v for k, v in means.items() if k != "Total"})
    return result + (meter_in.get_score(),) if compare_input else result


def validate_results(current, reference, best_metric=None):
    """evaluate_utils.py:121-151: is `current` better than `reference`? -> (bool, the better dict).  Compared over
    `best_metric` (a name or a list; all keys when it is empty or names none of them): RMSE must be lower, PSNR / SSIM
    higher, or the reference's value 0; other metrics do not vote.  Every vote must agree (no vote at all counts as
    agreement)."""
    if set(current) != set(reference):
        raise AssertionError(f"validate_results: different metrics {sorted(current)} / {sorted(reference)}")
    if isinstance(best_metric, str):
        best_metric = [best_metric]
    if not best_metric or all(x not in list(current.keys()) for x in best_metric):
        keys = list(current.keys())
    else:
        keys = best_metric
    votes = []
    for k in keys:
        if k.lower() in {"rmse"}:
            votes.append(current[k] < reference[k] or reference[k] == 0)
        if k.lower() in {"psnr", "ssim"}:
            votes.append(current[k] > reference[k] or reference[k] == 0)
    return (True, current) if all(votes) else (False, reference)


def do_eval(epochs, current_epoch, start_epochs, warmup_epochs, val_interval, val_start_epoch=1):
    """evaluate_utils.py:211-239: is it time to validate after epoch `current_epoch` (0-based)?  Always in the last
    epochs (current + 1 >= epochs - 3), in the first epoch after the warm-up, and every `val_interval` epochs (None:
    epochs // 10) from `val_start_epoch` on."""
    if val_interval is None:
        val_interval = epochs // 10
    if current_epoch + 1 >= epochs - 3:
        return True
    if start_epochs + warmup_epochs < current_epoch + 1 <= start_epochs + warmup_epochs + 1:
        return True
    return current_epoch + 1 >= val_start_epoch and (current_epoch + 1) % val_interval == 0
