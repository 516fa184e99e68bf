"""The training epoch of the reference's main.py on the device: `train_one_epoch`, `LossMonitor`, `EarlyStopper`,
`save_checkpoint` / `load_resume_state_dict`, `fit`.

Restates train/train_utils.py (EarlyStopper :12-81, get_tensor_range :84-96, get_gradient_range :127-143,
train_one_epoch :160-276), utils/utils.py (AverageMeter :40-64, get_loss_monitor :138-142, load_state_dict :352-370,
load_resume_state_dict :373-407) and main.py:123-258 without logging, plotting and tensorboard.

The reference's loop reads every loss term back with `.item()` every step (four host synchronisations per step with
MultiLoss) and, with `monitor_value: grad`, takes `.min()` / `.max()` of every parameter's gradient separately.  Here
the per-step values go into a device table, the gradient range comes out of the optimizer kernel (K11), and an epoch
synchronises once at its end -- the host keeps running ahead of the device, which is what hides its enqueue time.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .data import batch_pair
from .evaluate import do_eval, evaluate, validate_results
from .optim import tensor_ranges

MONITORS = ("grad", "input", "pred")


class LossMonitor:
    """get_loss_monitor's dict of AverageMeter (utils/utils.py:40-64, :138-142) for values that arrive as a table: the
    same Python-float arithmetic in the same order -- `sum += val * n; count += n; avg = sum / count` -- so the means
    equal the reference's bit for bit, given the same per-step fp32 values."""

    def __init__(self, names):
        self.names = list(names)
        self.reset()

    def reset(self):
        self.sum = {k: 0 for k in self.names}
        self.count = 0
        self.val = {k: 0 for k in self.names}

    def update(self, values, n=1):
        """values: {name: number} (a fp32 value is taken as the Python float `.item()` gives)."""
        for k in self.names:
            v = float(values[k])
            self.val[k] = v
            self.sum[k] += v * n
        self.count += n

    def update_rows(self, rows, weights):
        """rows: (steps, len(names)) array of per-step values, weights: the steps' batch sizes."""
        for row, n in zip(rows, weights):
            self.update({k: row[j] for j, k in enumerate(self.names)}, n)

    @property
    def avg(self):
        if self.count == 0:
            return {k: 0 for k in self.names}
        return {k: self.sum[k] / self.count for k in self.names}


class EarlyStopper:
    """EarlyStopper of train/train_utils.py:12-81, decisions included: it returns True once the compared value has failed
    to improve on its best by more than `min_delta` `patience` times in a row (patience None: never).

    The reference's quirk is kept by default: for `val_psnr`, `val_ssim` and `val_rmse` it STORES a monitored score
    (for `val_ssim` the PSNR) but COMPARES the `val_loss` argument, lower is better -- so those monitors behave like
    `val_loss`, except that they raise NotImplementedError when the score is missing from `eval_result`.  Checkpoints and
    logs are compared against reference runs, hence the default.  fixed=True compares the monitored score instead: RMSE
    lower is better, PSNR and SSIM higher is better.  `trainval_loss` counts the epochs whose validation loss exceeds the
    training loss by more than min_delta."""

    _SCORE = {"val_psnr": ("PSNR", "PSNR"), "val_ssim": ("SSIM", "PSNR"), "val_rmse": ("RMSE", "RMSE")}   # asked for, stored

    def __init__(self, patience, min_delta=1e-6, monitor="val_loss", fixed=False):
        self.patience, self.min_delta, self.monitor, self.fixed = patience, min_delta, monitor, bool(fixed)
        self.counter = 0
        self.min_val_loss = float("inf")
        self.val_loss = None
        self.train_loss = None

    def __call__(self, val_loss=None, train_loss=None, eval_result=None):
        if self.patience is None:
            return False
        compared = val_loss
        if self.monitor == "val_loss":
            self.val_loss = val_loss
        elif self.monitor == "trainval_loss":
            self.val_loss, self.train_loss = val_loss, train_loss
        elif self.monitor in self._SCORE and isinstance(eval_result, dict) and eval_result.get(self._SCORE[self.monitor][0]):
            asked, stored = self._SCORE[self.monitor]
            self.val_loss = eval_result[stored]
            if self.fixed:
                self.val_loss = eval_result[asked]
                compared = self.val_loss if asked == "RMSE" else -self.val_loss
        else:
            raise NotImplementedError
        if self.val_loss is None:
            return False
        if self.monitor == "trainval_loss":
            assert self.train_loss is not None, "train_loss must be provided"
            if val_loss > train_loss + self.min_delta:
                self.counter += 1
                if self.counter >= self.patience:
                    return True
            else:
                self.counter = 0
        else:
            if compared > self.min_val_loss + self.min_delta:
                self.counter += 1
                if self.counter >= self.patience:
                    return True
            else:
                self.min_val_loss = compared
                self.counter = 0
        return False


def _rows(n_hint, ncols, device):
    return torch.zeros((max(int(n_hint), 1), ncols), dtype=torch.float32, device=device)


def train_one_epoch(model, batches, criterion, optimizer, scheduler, reducer, model_name, input_data, monitor_value=(),
                    step=None, log_every=None):
    """train_one_epoch (train/train_utils.py:160-276) -> (mean Total loss, lr, {term: mean}, ranges).

    `model.train()`, then for each batch of `batches` (e.g. `data.RandomCropBatches`) the reference's loop body
    (:205-219): `criterion.reset()`, `data.batch_pair`, zero the gradients (`reducer.zero_grad()`), forward, criterion,
    `Total.backward()`, `reducer.finish()`, `optimizer.step()`; `scheduler.step()` once at the end.  `lr` is
    `optimizer.param_groups[0]["lr"]` read BEFORE that call, as the reference reads it.  A `reducer` of world > 1
    reduces the gradients in finish() as in any eager step.

    Every step's loss values (and ranges) go into one row of a device table; the epoch synchronises ONCE, with one
    device-to-host copy at its end.  log_every=N also fetches the rows so far every N steps and prints a progress line
    (each fetch is a synchronisation).  The means are formed on the host as AverageMeter forms them (`LossMonitor`),
    weighted with the batch sizes.

    monitor_value: any of "grad", "input", "pred" (the reference's `p.monitor_value`).  ranges[name] is a (steps, 3)
    float array of rows [min, max, count of non-finite elements]; "input" also gives ranges["gt"] (inputs[0] and the
    target, as the reference).  "grad" is the fused range of the optimizer step (`optimizer.grad_range`), started from the
    reference's 999 / -999: the min is never above 999, the max never below -999, and a step without any finite gradient
    reports [999, -999].  Where the reference's Python min() / max() over tensors keep or drop a NaN depending on the
    order of the parameters, min and max here are over the FINITE values and the count of the others stands beside them.

    step: a `graph.GraphedStep` built over the same model, reducer, optimizer and criterion.  The body then is
    `step(inputs, gt)`; only "Total" is reported (the graph's loss tensor; per-term values are not available under a
    graph), "grad" needs `optimizer.grad_range` to have been set BEFORE the capture (`optimizer.fused_grad_range()`), and
    "pred" is not available.

    A batch that carries "valid" (a store built with `hr_nodata` / `valid`, K19) is scored over its valid pixels:
    `criterion(pred, gt, valid=batch["valid"])`; the reported values are the masked ones.  With a GraphedStep such a batch
    raises NotImplementedError."""
    monitor_value = tuple(monitor_value or ())
    for m in monitor_value:
        if m not in MONITORS:
            raise ValueError(f"train_one_epoch: monitor_value {m!r} is not one of {MONITORS}")
    if step is not None:
        if "grad" in monitor_value and optimizer.grad_range is None:
            raise RuntimeError("train_one_epoch: monitor_value 'grad' with a GraphedStep needs optimizer.grad_range set before "
                               "the capture (optimizer.fused_grad_range()); the captured step does not write one")
        if "pred" in monitor_value:
            raise NotImplementedError("train_one_epoch: a GraphedStep does not hand out its prediction; monitor_value 'pred' "
                                      "is for the eager step")
    model.train()
    own_range = "grad" in monitor_value and optimizer.grad_range is None
    if own_range:
        optimizer.fused_grad_range()
    range_cols = [m2 for m in MONITORS if m in monitor_value for m2 in (("input", "gt") if m == "input" else (m,))]
    keys, table, weights, i = None, None, [], 0
    n_hint = len(batches) if hasattr(batches, "__len__") else 64
    try:
        for batch in batches:
            criterion.reset()
            inputs, gt, _base, _meta = batch_pair(batch, model_name, input_data)
            valid = batch.get("valid")
            if step is not None:
                if valid is not None:
                    raise NotImplementedError("train_one_epoch: a batch with a validity plane (a store built with hr_nodata / "
                                              "valid) and a GraphedStep: the masked graphed step is not built, use the eager step")
                values = [step(inputs, gt).detach().float().reshape(())]
                names, pred = ["Total"], None
            else:
                reducer.zero_grad()
                pred = model(*inputs)
                out = criterion(pred, gt) if valid is None else criterion(pred, gt, valid=valid)
                out["Total"].backward()
                reducer.finish()
                optimizer.step()
                names = list(out)
                values = [out[k].detach().float().reshape(()) for k in names]
            if keys is None:
                keys = names
                table = _rows(n_hint, len(keys) + 4 * len(range_cols), gt.device)
            elif i == table.shape[0]:                   # an iterable without a length: grow
                table = torch.cat([table, torch.zeros_like(table)])
            row = table[i]
            row[:len(keys)] = torch.stack(values)
            c = len(keys)
            for name in range_cols:
                if name == "grad":
                    row[c:c + 4] = optimizer.grad_range
                elif name == "input":
                    tensor_ranges([inputs[0], gt], table=row[c:c + 8].view(2, 4))
                elif name == "pred":
                    tensor_ranges([pred.detach()], table=row[c:c + 4].view(1, 4))
                c += 4
            weights.append(int(gt.size(0)))
            i += 1
            if log_every and i % int(log_every) == 0:
                host = table[:i].cpu().numpy()
                mon = LossMonitor(keys)
                mon.update_rows(host[:, :len(keys)], weights)
                print(f"step {i}: loss {mon.avg['Total']:5.3e} lr {float(optimizer.param_groups[0]['lr']):4.2e}", flush=True)
    finally:
        if own_range:
            optimizer.grad_range = None
    if keys is None:
        raise ValueError("train_one_epoch: no batches")
    lr = float(optimizer.param_groups[0]["lr"])
    scheduler.step()
    host = table[:i].cpu().numpy()               # the epoch's one synchronisation
    monitor = LossMonitor(keys)
    monitor.update_rows(host[:, :len(keys)], weights)
    means = monitor.avg
    ranges, c = {}, len(keys)
    for name in range_cols:
        ranges[name] = host[:, c:c + 3].astype(np.float64)
        c += 4
    return means["Total"], lr, {k: v for k, v in means.items() if k != "Total"}, ranges


def load_state_dict(model, state_dict):
    """load_state_dict of utils/utils.py:352-370: copy the entries whose key and size match the model's, keep the rest."""
    own = model.state_dict()
    own.update({k: v for k, v in state_dict.items() if k in own and v.size() == own[k].size()})
    model.load_state_dict(own)
    ops.invalidate_packed_weights()
    return model


def save_checkpoint(path, model, optimizer, scheduler, epoch, best_result):
    """The checkpoint main.py:246-252 writes with every improved model: {"optimizer" (the matching torch.optim class's
    layout, so the reference's loop can resume from it), "state_dict", "scheduler", "epoch", "best_result"}."""
    try:
        opt_sd = optimizer.state_dict(layout="torch")
    except TypeError:                            # a torch optimizer
        opt_sd = optimizer.state_dict()
    torch.save({"optimizer": opt_sd, "state_dict": model.state_dict(), "scheduler": scheduler.state_dict(),
                "epoch": int(epoch), "best_result": best_result}, path)


def load_resume_state_dict(model, optimizer, scheduler, path, resume=False):
    """load_resume_state_dict of utils/utils.py:373-407 -> (model, start_epoch, best_result, optimizer, scheduler): the
    weights are always loaded (`load_state_dict` above); epoch, optimizer and scheduler state only with resume=True
    (start_epoch 0 and scheduler None otherwise, as there).  The optimizer entry may be in torch's layout (what the
    reference and `save_checkpoint` write) or the flat one."""
    ck = torch.load(path, map_location="cpu")
    start_epoch = ck["epoch"] if resume else 0
    model = load_state_dict(model, ck["state_dict"])
    if optimizer is not None and resume:
        optimizer.load_state_dict(ck["optimizer"])
    if scheduler is not None and resume:
        scheduler.load_state_dict(ck["scheduler"])
    else:
        scheduler = None
    return model, start_epoch, ck["best_result"], optimizer, scheduler


def _get(mapping, key, default=None):
    if isinstance(mapping, dict):
        return mapping.get(key, default)
    return getattr(mapping, key, default)


def fit(p, model, train_batches, val_batches, criterion, optimizer, scheduler, reducer, meter, checkpoint_path=None,
        resume_from=None, step=None):
    """main.py:123-258 without logging and plotting -> the history, a list of dicts.

    p (attributes or keys, the reference's names): epochs, model_name, input_data, scheduler_kwargs {warmup_epoch},
    val_interval, val_start_epoch (1), best_metric, early_stop {patience, monitor}, monitor_value, resume.
    resume_from: a checkpoint (`p.model_kwargs.checkpoint` there) loaded with `load_resume_state_dict(..., p.resume)`.
    Then the initial evaluation (`evaluate(..., compare_input=True)`; its scores are the first "best"), and for every
    epoch `train_one_epoch`, and where `do_eval` says so `evaluate`, `validate_results` against the best so far, the
    checkpoint of an improved model (`save_checkpoint` to checkpoint_path, if given; "{epoch}" in it is replaced by the
    1-based epoch, which keeps every improved model instead of the last) and, after epoch 200 only,
    `EarlyStopper(patience, 1e-4, monitor)`.

    history[0] is the initial evaluation {"epoch": start_epoch, "scores", "val_loss", "input_scores"}; every later entry
    is one epoch {"epoch" (1-based), "train_loss", "lr", "terms", "ranges", "evaluated"} plus, where evaluated, "scores",
    "val_loss", "is_better", "best", and "stopped" on the epoch the stopper ended the run.

    A store whose ground truth has voids (`DeviceScenes(hr_nodata=)`, K19: its batches carry "valid") is fitted with a
    meter built with `masked=True` (K20): the criterion and both meters then see the plane, the scores are over valid pixels
    and `meter.counts()` holds the last evaluation's per-tile counts.  Any other meter raises NotImplementedError in the
    initial evaluation."""
    epochs = int(_get(p, "epochs"))
    name, input_data = _get(p, "model_name"), _get(p, "input_data")
    start_epoch = 0
    if resume_from is not None:
        model, start_epoch, _best, _, _ = load_resume_state_dict(model, optimizer, scheduler, resume_from, bool(_get(p, "resume")))
    best, val_loss, _terms, input_scores = evaluate(model, val_batches, criterion, meter, name, input_data, compare_input=True)
    history = [{"epoch": start_epoch, "scores": dict(best), "val_loss": val_loss, "input_scores": input_scores}]
    early = _get(p, "early_stop") or {}
    stopper = EarlyStopper(patience=_get(early, "patience", None), min_delta=1e-4, monitor=_get(early, "monitor", "val_loss"))
    warmup = _get(_get(p, "scheduler_kwargs") or {}, "warmup_epoch", 0) or 0
    val_start = _get(p, "val_start_epoch")
    for epoch in range(start_epoch, epochs):
        train_loss, lr, terms, ranges = train_one_epoch(model, train_batches, criterion, optimizer, scheduler, reducer, name,
                                                        input_data, monitor_value=_get(p, "monitor_value") or (), step=step)
        entry = {"epoch": epoch + 1, "train_loss": train_loss, "lr": lr, "terms": terms, "ranges": ranges, "evaluated": False}
        history.append(entry)
        if do_eval(epochs, epoch, start_epoch, warmup, _get(p, "val_interval"), 1 if val_start is None else val_start):
            scores, val_loss, _terms = evaluate(model, val_batches, criterion, meter, name, input_data)
            is_better, best = validate_results(scores, best, _get(p, "best_metric"))
            entry.update(evaluated=True, scores=scores, val_loss=val_loss, is_better=is_better, best=dict(best))
            if is_better and checkpoint_path is not None:
                save_checkpoint(str(checkpoint_path).format(epoch=epoch + 1), model, optimizer, scheduler, epoch + 1, best)
            if epoch > 200 and stopper(val_loss, train_loss, scores):
                entry["stopped"] = True
                break
    return history
