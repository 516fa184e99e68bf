"""One validation pass timed two ways on the same commit, and K10 (`metrics.batch_scores`) on its own.

Workload: the benched architecture in eval mode (JSPSR, image + mask, num_feature 32), bf16 and fp32 storage, 1 024 tiles
of 128 x 128 cut from synthetic 334 x 334 scenes (9 tiles per scene, configs' val set-up: log-scaled relative DEMs,
val_border 0.05), criterion L1 + L2 + 0.1 Grad, the five configured metrics (PSNR piq, RMSE, Median, NMAD, LE95).
  * batched: `evaluate.evaluate` over `TileCropBatches(batch_size=50)`: one K10 launch per batch, one host
    synchronisation per pass;
  * tile loop: what the one-tile API allows -- `TileCropBatches(batch_size=1)`, forward, criterion, `Meter.update`
    (26 launches per tile), `.item()` on every loss value per tile as the reference's eval_model does.
Each leg is warmed up, then the two are run alternately `--reps` times; host clock around a pass that ends in a device
synchronise.  Reported: every repetition, the median and the min-max spread.  Both passes' scores are compared.
Then `batch_scores` alone at B = 1, 50, 256 against B calls of `tile_scores` on the same tiles (device events around
`iters` repetitions, after a warm-up), again alternating.
Usage: python tools/bench_eval.py [--tiles N] [--reps R] [--nf F] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jspsr_amd import _lib  # noqa: E402
from jspsr_amd import data as D  # noqa: E402
from jspsr_amd import evaluate as EV  # noqa: E402
from jspsr_amd import losses as L  # noqa: E402
from jspsr_amd import metrics as M  # noqa: E402
from tests import batches_ref as R  # noqa: E402

P = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True, scale_mask=True)
IC = {"lr_dem": 1, "image": 3, "mask": 15}
METRICS = {"PSNR": {"package": "piq"}, "RMSE": {"package": "local"}, "Median": {"package": "local"},
           "NMAD": {"package": "local"}, "LE95": {"package": "local"}}
LOSS = {"L1": 1, "L2": 1, "Grad": 0.1}
BORDER = 0.05


def spread(xs):
    return f"median {statistics.median(xs):9.2f}  min {min(xs):9.2f}  max {max(xs):9.2f}  (n={len(xs)}: " + \
        " ".join(f"{x:.1f}" for x in xs) + ")"


def batched_pass(model, S, bs):
    meter = EV.PerformanceMeter(METRICS, P["elev_min"], P["elev_max"], border=BORDER, elev_log=P["elev_log"])
    return EV.evaluate(model, D.TileCropBatches(S, bs, 128, 9), L.get_criterion(LOSS), meter, "JSPSR", IC)


@torch.no_grad()
def tile_loop_pass(model, S):
    model.eval()
    meter, crit = M.Meter(P["elev_min"], P["elev_max"], border=BORDER, elev_log=P["elev_log"]), L.get_criterion(LOSS)
    sums, n = {}, 0
    for b in D.TileCropBatches(S, 1, 128, 9):
        crit.reset()
        inputs, gt, _, _ = D.batch_pair(b, "JSPSR", IC)
        pred = model(*inputs)
        for k, v in crit(pred, gt).items():
            sums[k] = sums.get(k, 0.0) + v.item()
        meter.update(pred, gt)
        n += 1
    return meter.scores(), sums["Total"] / n, {k: v / n for k, v in sums.items() if k != "Total"}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nf", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_eval needs the MI355X"
    lib = _lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from jspsr_amd.JSPSR import Model
    n_sc = (args.tiles + 8) // 9
    scenes = R.make_scenes([(334, 334)] * n_sc, seed=1)
    S = D.DeviceScenes(**{k: [s[k] for s in scenes] for k in ("lr_dem", "hr_dem", "image", "mask")}, device="cuda", **P)
    n_tiles = n_sc * 9
    torch.manual_seed(0)
    model = Model(dict(IC, COP30=1), num_feature=args.nf).to("cuda").eval()
    say(f"# validation pass: JSPSR image+mask nf {args.nf}, eval mode, {n_tiles} tiles of 128 x 128 ({n_sc} scenes x 9), "
        f"border {BORDER}, log scaling; {torch.cuda.get_device_name(0)}")
    say("# ms per pass, host clock around a pass ended by a device synchronise; legs alternate within a repetition")
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        model.compute_dtype = dtype
        batched_pass(model, S, 50)                                    # warm-up: every shape both legs use
        tile_loop_pass(model, S)
        tb, tl = [], []
        for _ in range(args.reps):
            t, rb = timed(lambda: batched_pass(model, S, 50))
            tb.append(t)
            t, rl = timed(lambda: tile_loop_pass(model, S))
            tl.append(t)
        say(f"{tag} evaluate(), batch 50 : {spread(tb)}")
        say(f"{tag} tile loop, batch 1  : {spread(tl)}")
        say(f"{tag} ratio of medians (tile loop / batched): {statistics.median(tl) / statistics.median(tb):.2f}")
        diff = {k: abs(rb[0][k] - rl[0][k]) for k in rb[0]}
        say(f"{tag} scores batched {({k: round(v, 5) for k, v in rb[0].items()})}")
        say(f"{tag} |batched - tile loop| per score {({k: float(f'{v:.2e}') for k, v in diff.items()})}; Total loss {rb[1]:.6f} / {rl[1]:.6f}")
    # K10 alone
    say()
    say("# batch_scores (K10, one launch) vs B calls of tile_scores (26 launches each), us per B tiles of 128 x 128, device events")
    g = torch.Generator().manual_seed(1)
    for B in (1, 50, 256):
        gt = torch.rand(B, 1, 128, 128, generator=g) * 0.5 + 0.2
        pred = (gt + 0.004 * torch.randn(B, 1, 128, 128, generator=g)).cuda()
        gt = gt.cuda()
        one = lambda: M.batch_scores(pred, gt, P["elev_min"], P["elev_max"], BORDER, True)          # noqa: E731
        many = lambda: [M.tile_scores(pred[b:b + 1], gt[b:b + 1], P["elev_min"], P["elev_max"], BORDER, True) for b in range(B)]  # noqa: E731
        for _ in range(5):
            one()
        many()
        torch.cuda.synchronize()
        n0 = lib.jspsr_launch_count(b"scores_batch (lds)")
        one()
        assert lib.jspsr_launch_count(b"scores_batch (lds)") == n0 + 1
        iters_one, iters_many = max(20, 2000 // B), max(3, 200 // B)
        a, b_ = [], []
        for _ in range(args.reps):
            a.append(events(one, iters_one))
            b_.append(events(many, iters_many))
        say(f"B = {B:3d} batch_scores : {spread(a)}")
        say(f"B = {B:3d} tile_scores x B: {spread(b_)}")
        say(f"B = {B:3d} ratio of medians: {statistics.median(b_) / statistics.median(a):.1f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
