"""K15 (tiled whole-scene inference, jspsr_amd/infer.py) on one MI355X.

  launches    `infer.prepare_windows` and `infer.merge_windows` (one launch each) for the whole cover of a scene against the
              same work done with what the package offered before: the decoded rasters sliced per tile on the host
              (numpy), a store of the tiles (`InferenceScenes`, one upload), `infer.prepare` on it; and `infer.finish`
              (metres per tile), a download, and the feather merge in numpy (tests/tiled_ref.py).  A host clock around calls
              that end in a synchronise -- the old way has host work in it -- warmed up, windows of at least 0.1 s of K15's
              calls (3 calls of the old way), the two legs alternating within a repetition; median, min and max of the
              repetitions, in ms with three decimals.  The new leg is also timed by device events alone; its bytes/s are
              on the algorithmic count: prepare reads 22 B and writes 76 B per window pixel, merge reads 4 B per tile value
              of non-zero weight and writes 4 B per scene pixel.
              Reported, not gated.
  end to end  `predict_scenes(model, scenes, batch_size=8)` untiled against `tile=512, overlap=64, trim=16`, JSPSR image +
              mask, 32 features, fp32: time per pass and `torch.cuda.max_memory_allocated` of a pass after a reset of the
              peak.  The tiled pass recomputes the overlaps, about (k / (k - overlap))^2 of the untiled work; its peak
              follows batch_size x tile^2.  The two results are NOT equal (per-tile channel-gate statistics, zero padding
              at tile edges); their difference is printed.  The untiled pass is run only up to --untiled-limit frame pixels
              (default 768 x 4096, the largest frame a convolution kernel of the package is tested on).
  scenes      2048 x 2048 and 1024 x 768; --large SIDE adds one tiled pass over a SIDE x SIDE scene (no untiled leg).
Usage: python tools/bench_tiled_infer.py [--reps R] [--no-model] [--large SIDE] [--untiled-limit PIXELS] [--out FILE]"""
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
WINDOW = 0.1                # seconds of K15's calls in one timed window


def spread(xs, unit="ms"):
    return f"median {statistics.median(xs):10.3f}  min {min(xs):10.3f}  max {max(xs):10.3f} {unit} (n={len(xs)})"


def big_scene(R, np, h, w, seed):
    """One decoded scene of h x w: a 512 x 512 synthetic scene repeated (the kernels do not care), the DEM with a slope on
    top so that the tiles differ."""
    s = R.make_scenes([(min(h, 512), min(w, 512))], seed=seed)[0]
    reps = (-(-h // 512), -(-w // 512), 1)
    out = {k: np.ascontiguousarray(np.tile(s[k], reps)[:h, :w]) for k in KINDS}
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out["lr_dem"] = (out["lr_dem"] + (0.01 * yy + 0.005 * xx)[..., None]).astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--large", type=int, default=0)
    ap.add_argument("--untiled-limit", type=int, default=768 * 4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import infer as I
    from tests import batches_ref as R
    from tests import tiled_ref as TR
    assert torch.cuda.is_available(), "bench_tiled_infer needs the MI355X"
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def clock(fn, iters=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3, out

    model = None
    if not args.no_model:
        from jspsr_amd.JSPSR import Model
        torch.manual_seed(0)
        model = Model(dict(IC, COP30=1), num_feature=32).to(dev).eval()
    say(f"# K15, tiled whole-scene inference; {torch.cuda.get_device_name(0)}; tile {TILE}, overlap {OVERLAP}, trim {TRIM}, "
        f"batch {BATCH}")
    shapes = [(2048, 2048), (1024, 768)] + ([(args.large, args.large)] if args.large else [])
    for n, (h, w) in enumerate(shapes):
        large = bool(args.large) and n == len(shapes) - 1
        scene = big_scene(R, np, h, w, seed=n + 1)
        S = I.InferenceScenes(**{k: [scene[k]] for k in KINDS}, device=dev, **P)
        cover = I.plan_cover(h, w, TILE, OVERLAP, TRIM)
        windows = [(0, y, x) for y, x in cover.windows()]
        say()
        say(f"# scene {h} x {w}: {cover.n_y} x {cover.n_x} = {cover.n} tiles, {cover.n * TILE * TILE / (h * w):.2f} x the scene's pixels"
            f" ((k / (k - overlap))^2 = {(TILE / (TILE - OVERLAP)) ** 2:.2f})")
        if not large:
            pred = (torch.rand((cover.n, 1, TILE, TILE), generator=torch.Generator().manual_seed(2)) * 1.2 - 0.1).to(dev)
            base = [S.base[0]] * cover.n
            ref_cover = TR.cover(h, w, TILE, OVERLAP, TRIM)

            def old_prepare():
                cut = {k: [np.ascontiguousarray(scene[k][y:y + TILE, x:x + TILE]) for _, y, x in windows] for k in KINDS}
                tiles = I.InferenceScenes(**cut, device=dev, base=base, **P)
                return I.prepare(tiles, list(range(cover.n)), 0, 8)[0], tiles

            def old_merge(tiles):
                m = I.finish(pred, tiles, list(range(cover.n)), I.Frame(TILE, TILE, 0, 0, TILE, TILE)).cpu().numpy()
                return TR.merge(m, ref_cover)

            new_prepare = lambda: I.prepare_windows(S, windows, TILE)                       # noqa: E731
            new_merge = lambda: I.merge_windows(pred, S, [0], cover)                        # noqa: E731
            (old_inputs, tile_store), got = old_prepare(), new_prepare()
            assert all(torch.equal(a, b) for a, b in zip(got, old_inputs)), "prepare_windows differs from prepare on a store of tiles"
            assert np.array_equal(new_merge()[0].cpu().numpy(), old_merge(tile_store)), "merge_windows differs from the numpy merge"
            del old_inputs, got
            # tile values the merge reads: one per (tile, pixel) of non-zero weight -- separable, so a product of two counts
            reads = int((cover.wy != 0).sum()) * int((cover.wx != 0).sum())
            legs = {"prepare": (new_prepare, lambda: old_prepare()[0], cover.n * TILE * TILE * (76 + 22)),
                    "merge": (new_merge, lambda: old_merge(tile_store), reads * 4 + h * w * 4)}
            say("# ms per call: a host clock around a call and a synchronise; the legs alternate within a repetition")
            for name, (new, old, nbytes) in legs.items():
                for _ in range(2):
                    new()
                    old()
                iters = max(10, int(WINDOW / (clock(new, 10)[0] * 1e-3)))                    # WINDOW seconds of K15's calls
                t_new, t_old, t_dev = [], [], []
                for _ in range(args.reps):
                    t_new.append(clock(new, iters)[0])
                    t_old.append(clock(old, 3)[0])
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        new()
                    e1.record()
                    torch.cuda.synchronize()
                    t_dev.append(e0.elapsed_time(e1) / iters)
                say(f"{name:8s} K15, 1 launch          {spread(t_new)}  ({iters} calls per window)")
                say(f"{name:8s} K15, device events     {spread(t_dev)}  {nbytes / (statistics.median(t_dev) * 1e-3) / 1e9:8.1f} GB/s on "
                    f"{nbytes / 1e6:.1f} MB")
                say(f"{name:8s} host slices + K13 + numpy {spread(t_old)}  x{statistics.median(t_old) / statistics.median(t_new):.1f}")
            del pred, tile_store
        if model is not None:
            passes = {"tiled": lambda: I.predict_scenes(model, S, batch_size=BATCH, tile=TILE, overlap=OVERLAP, trim=TRIM)}
            if not large and h * w <= args.untiled_limit:
                passes["untiled"] = lambda: I.predict_scenes(model, S, batch_size=BATCH)
            else:
                say(f"untiled  NOT RUN: {h * w} frame pixels are past --untiled-limit {args.untiled_limit}")
            results = {}
            for name, one in passes.items():
                one()                                                                       # warm: weights packed, tables cached
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                ts, same = [], "one pass"
                for _ in range(1 if large else args.reps):
                    t, r = clock(one)
                    if ts:
                        same = f"the last two passes bit-equal: {torch.equal(r.buffer.view(torch.int32), results[name].view(torch.int32))}"
                    ts.append(t)
                    results[name] = r.buffer
                peak = torch.cuda.max_memory_allocated()
                say(f"{name:8s} predict_scenes, JSPSR nf-32 fp32: {spread(ts)}  {h * w / statistics.median(ts) / 1e3:7.1f} Mpixel/s;  "
                    f"peak {peak / 2 ** 20:9.1f} MiB allocated ({(peak - before) / 2 ** 20:.1f} MiB above the {before / 2 ** 20:.1f} MiB "
                    f"held before the pass); finite: {bool(torch.isfinite(r.buffer).all())}; {same}")
                del r
            if len(results) == 2:
                d = (results["tiled"] - results["untiled"]).abs()
                say(f"tiled against untiled (not an exact decomposition): max |difference| {float(d.max()):.3f} m, mean "
                    f"{float(d.mean()):.4f} m")
            del results
        del S, scene
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
