"""K16 (the self-ensemble per window of a tiled scene, jspsr_amd/infer.py) on one MI355X.

  kernels     `infer.prepare_windows_d4` for one element at a time -- an even one (a half turn; a mirror image) and an odd one
              (a quarter turn; a quarter turn with a mirror image) -- against `infer.prepare_windows` (K15, upright) on
              the same windows: the windows of the cover of a 2048 x 2048 scene at tile 512, one launch each, the same
              bytes in every leg (22 B read and 76 B written per window pixel, image + mask).  Device events around a
              window of at least 0.1 s of calls, warmed up, the legs alternating within a repetition; median, min and max
              of the repetitions in ms with three decimals, bytes/s on the algorithmic count, and the ratio to the upright
              kernel of the same run (upright time / leg time: below 1 is slower).  `infer.mean_windows` is timed the same
              way (K reads and one fp32 write per tile pixel).  Reported, not gated.
  whole pass  `predict_scenes(model, scenes, batch_size=8, tile=512, overlap=64, trim=16, window_tta="d4")` against the plain
              tiled pass and against the composition by hand -- `prepare_windows`, torch.rot90 / torch.flip on the device,
              the model in the same batches, `mean_windows`, `merge_windows` --, JSPSR image + mask, 32 features, fp32: a
              host clock around a pass that ends in a synchronise, and `torch.cuda.max_memory_allocated` of a pass after
              a reset of the peak.  The by-hand result must be bit-equal to predict_scenes'.
  scenes      2048 x 2048 and 1024 x 768.
Usage: python tools/bench_window_tta.py [--reps R] [--no-model] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True, scale_mask=True)
IC = {"lr_dem": 1, "image": 3, "mask": 15}
KINDS = ("lr_dem", "image", "mask")
TILE, OVERLAP, TRIM, BATCH = 512, 64, 16, 8
WINDOW = 0.1                # seconds of calls in one timed window
LEGS = [("upright (K15)", None), ("even  (2, F, F)", (2, False, False)), ("even  (0, T, F)", (0, True, False)),
        ("odd   (1, F, F)", (1, False, False)), ("odd   (3, T, F)", (3, True, False))]


def spread(xs, unit="ms"):
    return f"median {statistics.median(xs):10.3f}  min {min(xs):10.3f}  max {max(xs):10.3f} {unit} (n={len(xs)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import infer as I
    from tests import batches_ref as R
    from tools.bench_tiled_infer import big_scene
    assert torch.cuda.is_available(), "bench_window_tta needs the MI355X"
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def clock(fn):
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
        return e0.elapsed_time(e1) / iters

    def turned(t, e):
        t = torch.rot90(t, e[0], dims=(-2, -1))
        t = torch.flip(t, dims=(-1,)) if e[1] else t
        return (torch.flip(t, dims=(-2,)) if e[2] else t).contiguous()

    def by_hand(model, S, cover, elements, batch):
        """predict_scenes' schedule from the public pieces, the transforms by torch on the device."""
        windows = [(0, y, x) for y, x in cover.windows()]
        nb = max(1, batch // len(elements))
        per = max(1, batch // nb)
        order = [e for e in elements if e[0] % 2 == 0] + [e for e in elements if e[0] % 2 == 1]      # a square tile: one set
        means = []
        with torch.no_grad():
            for lo in range(0, len(windows), nb):
                up = I.prepare_windows(S, windows[lo:lo + nb], TILE)
                n, preds = up[0].shape[0], {}
                for e0 in range(0, len(order), per):
                    run = order[e0:e0 + per]
                    pred = model(*[torch.cat([turned(t, e) for e in run]) for t in up])
                    for j, e in enumerate(run):
                        preds[e] = pred[j * n:(j + 1) * n]
                means.append(I.mean_windows([preds[e] for e in elements], elements, TILE))
        return I.merge_windows(torch.cat(means), S, [0], cover)

    model = None
    if not args.no_model:
        from jspsr_amd.JSPSR import Model
        torch.manual_seed(0)
        model = Model(dict(IC, COP30=1), num_feature=32).to(dev).eval()
    elements = I.d4_elements("d4")
    say(f"# K16, the self-ensemble per window; {torch.cuda.get_device_name(0)}; tile {TILE}, overlap {OVERLAP}, trim {TRIM}, "
        f"batch {BATCH}")
    for n, (h, w) in enumerate([(2048, 2048), (1024, 768)]):
        scene = big_scene(R, np, h, w, seed=n + 1)
        S = I.InferenceScenes(**{k: [scene[k]] for k in KINDS}, device=dev, **P)
        cover = I.plan_cover(h, w, TILE, OVERLAP, TRIM)
        windows = [(0, y, x) for y, x in cover.windows()]
        say()
        say(f"# scene {h} x {w}: {cover.n_y} x {cover.n_x} = {cover.n} tiles")
        if n == 0:
            calls = {name: ((lambda: I.prepare_windows(S, windows, TILE)) if e is None else
                            (lambda e=e: I.prepare_windows_d4(S, windows, TILE, [e]))) for name, e in LEGS}
            up = I.prepare_windows(S, windows, TILE)
            for name, e in LEGS[1:]:
                (got, _), = calls[name]().values()
                assert all(torch.equal(a, turned(b, e)) for a, b in zip(got, up)), f"{name} differs from the torch transform"
            del up, got
            nbytes = cover.n * TILE * TILE * (76 + 22)
            say(f"# prepare: ms per launch by device events, {cover.n} windows per launch, {nbytes / 1e6:.1f} MB; the legs alternate "
                f"within a repetition")
            for fn in calls.values():
                for _ in range(3):
                    fn()
            iters = max(10, int(WINDOW / (events(calls[LEGS[0][0]], 10) * 1e-3)))
            ts = {name: [] for name in calls}
            for _ in range(args.reps):
                for name, fn in calls.items():
                    ts[name].append(events(fn, iters))
            ref = statistics.median(ts[LEGS[0][0]])
            for name, t in ts.items():
                say(f"prepare {name:16s} {spread(t)}  {nbytes / (statistics.median(t) * 1e-3) / 1e9:8.1f} GB/s  "
                    f"upright / this = {ref / statistics.median(t):.2f}  ({iters} calls per window)")
            g = torch.Generator().manual_seed(3)
            for K in (2, 8):
                preds = [(torch.rand((cover.n, 1, TILE, TILE), generator=g) * 1.2 - 0.1).to(dev) for _ in range(K)]
                mean = lambda: I.mean_windows(preds, elements[:K], TILE)                     # noqa: E731
                for _ in range(3):
                    mean()
                it = max(10, int(WINDOW / (events(mean, 10) * 1e-3)))
                t = [events(mean, it) for _ in range(args.reps)]
                mb = cover.n * TILE * TILE * 4 * (K + 1)
                say(f"mean_windows K = {K}        {spread(t)}  {mb / (statistics.median(t) * 1e-3) / 1e9:8.1f} GB/s on {mb / 1e6:.1f} MB"
                    f"  ({it} calls per window)")
            del preds
        if model is not None:
            kw = dict(batch_size=BATCH, tile=TILE, overlap=OVERLAP, trim=TRIM)
            passes = {"plain tiled": lambda: I.predict_scenes(model, S, **kw).buffer,
                      "window_tta d4": lambda: I.predict_scenes(model, S, window_tta="d4", **kw).buffer,
                      "by hand, torch": lambda: by_hand(model, S, cover, elements, BATCH).view(-1)}
            results, medians = {}, {}
            for name, one in passes.items():
                one()                                                                       # warm: weights packed, tables cached
            for name, one in passes.items():
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                ts, same = [], "one pass"
                for _ in range(args.reps):
                    t, r = clock(one)
                    if ts:
                        same = f"the last two passes bit-equal: {torch.equal(r.view(torch.int32), results[name].view(torch.int32))}"
                    ts.append(t)
                    results[name] = r
                peak = torch.cuda.max_memory_allocated()
                medians[name] = statistics.median(ts)
                say(f"{name:15s} JSPSR nf-32 fp32: {spread(ts)}  {h * w / statistics.median(ts) / 1e3:7.1f} Mpixel/s;  "
                    f"peak {peak / 2 ** 20:9.1f} MiB allocated ({(peak - before) / 2 ** 20:.1f} MiB above the {before / 2 ** 20:.1f} MiB "
                    f"held before the pass); finite: {bool(torch.isfinite(r).all())}; {same}")
                del r
            d = (results["window_tta d4"] - results["plain tiled"]).abs()
            say(f"window_tta / plain tiled = {medians['window_tta d4'] / medians['plain tiled']:.2f} x (K = {len(elements)});  "
                f"window_tta / by hand = {medians['window_tta d4'] / medians['by hand, torch']:.2f} x;  by hand bit-equal to "
                f"predict_scenes: {torch.equal(results['window_tta d4'].view(torch.int32), results['by hand, torch'].view(torch.int32))};  "
                f"ensemble against single pass: max |difference| {float(d.max()):.3f} m, mean {float(d.mean()):.4f} m")
            del results
        del S, scene
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
