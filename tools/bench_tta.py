"""K14 (whole-scene self-ensemble, jspsr_amd/infer.py: prepare_d4, finish_mean, predict_scenes(tta=...)) on one MI355X.

  prepare     `prepare_d4` of the four quarter-turn elements (rot90 1, 3: 32 x 32 tiles staged in LDS) against the four
              upright ones (rot90 0, 2: K13's row-wise gather with reversed indices): the same scenes, the same number of
              samples and frame pixels, one launch each.  Also K13's `prepare` of the same scenes repeated four times, the
              launch both are measured against.
  finish      `finish_mean` with the eight elements (ONE launch: inverse transforms, mean, metres) against eight
              `finish` launches on the same eight predictions (which leave the inverse transforms and the mean undone).
              Both: device events around windows of at least 0.1 s of calls, warmed up, the legs alternating within a
              repetition; median, min and max of the repetitions.
  end to end  `predict_scenes(tta="d4")` + `rasters()` against what a user of K13 alone has to do: np.rot90 / fliplr of every
              decoded raster, eight `InferenceScenes` uploads, eight `predict_scenes(metres=False)` + `rasters()`, the
              inverse transforms, the fp32 mean and the metre conversion in numpy.  A host clock around whole passes (both
              end in a device-to-host copy); batch_size 8 in both legs: the same forward shapes on workload 1, while on
              workload 2 the by-hand forwards are single samples against four variants of the one scene.
  workload 1  8 scenes of 334 x 334, pad 89 (cal_pad: a 512 x 512 frame), image + mask, JSPSR 32 features, bf16
  workload 2  one 1024 x 768 scene, pad 0 (frames 1024 x 768 and 768 x 1024), image + mask, the same model
No number here is gated: the file states what was measured.
Usage: python tools/bench_tta.py [--reps R] [--workloads 1,2] [--no-model] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True, scale_mask=True)
IC = {"lr_dem": 1, "image": 3, "mask": 15}
KINDS = ("lr_dem", "image", "mask")
WINDOW = 0.1                # seconds of calls in one timed window


def spread(xs, unit="us"):
    return f"median {statistics.median(xs):10.1f}  min {min(xs):10.1f}  max {max(xs):10.1f} {unit} (n={len(xs)})"


def events(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="1,2")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import infer as I
    from tests import batches_ref as R
    assert torch.cuda.is_available(), "bench_tta needs the MI355X"
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def alternate(legs, floor_iters):
        """{name: fn} -> {name: [us per call per repetition]}; the window sized on the first leg."""
        for fn in legs.values():
            for _ in range(3):
                fn()
        first = next(iter(legs.values()))
        iters = max(floor_iters, int(WINDOW / (events(torch, first, floor_iters) * 1e-6)))
        for fn in legs.values():
            events(torch, fn, floor_iters)
        ts = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                ts[name].append(events(torch, fn, iters))
        return ts, iters

    elements = I.d4_elements("d4")
    even, odd = [e for e in elements if e[0] % 2 == 0], [e for e in elements if e[0] % 2 == 1]
    say(f"# K14, whole-scene self-ensemble; {torch.cuda.get_device_name(0)}")
    for wl in [int(w) for w in args.workloads.split(",")]:
        n_scenes, (H, W), pad = ((8, (334, 334), 89), (1, (1024, 768), 0))[wl - 1]
        scenes = R.make_scenes([(H, W)] * n_scenes, seed=wl, coord=False)
        S = I.InferenceScenes(**{k: [s[k] for s in scenes] for k in KINDS}, device=dev, **P)
        idx = list(range(n_scenes))
        groups = I.prepare_d4(S, idx, elements, pad, 8)
        fe, fo = groups[0][1], groups[1][1]
        say()
        say(f"# workload {wl}: {n_scenes} scene(s) of {H} x {W}, pad {pad} -> frames {fe.Hp} x {fe.Wp} (rot90 0, 2) and "
            f"{fo.Hp} x {fo.Wp} (rot90 1, 3), image + mask; us per call, device events around windows of at least {WINDOW} s, "
            f"legs alternate within a repetition")
        # -- prepare: 4 elements x n_scenes samples per launch in every leg
        nbytes = 4 * n_scenes * (fe.Hp * fe.Wp * 76 + H * W * 22)              # written per frame pixel, read per source pixel
        ts, iters = alternate({"even": lambda: I.prepare_d4(S, idx, even, pad, 8),
                               "odd": lambda: I.prepare_d4(S, idx, odd, pad, 8),
                               "k13": lambda: I.prepare(S, idx * 4, pad, 8)}, 20)
        m = {k: statistics.median(v) for k, v in ts.items()}
        for name, what in (("even", "prepare_d4 rot90 0, 2"), ("odd", "prepare_d4 rot90 1, 3"), ("k13", "K13 prepare, 4 x the scenes")):
            say(f"prepare  {what:28s} 1 launch  {spread(ts[name])}  {nbytes / (m[name] * 1e-6) / 1e9:8.1f} GB/s on {nbytes / 1e6:.1f} MB")
        say(f"prepare  {iters} calls per window; odd / even = x{m['odd'] / m['even']:.3f}; even / K13 = x{m['even'] / m['k13']:.3f}; "
            f"odd / K13 = x{m['odd'] / m['k13']:.3f}")
        # -- finish: eight predictions -> one result
        g = torch.Generator().manual_seed(3)
        preds = [(torch.rand((n_scenes, 1, (fo if e[0] % 2 else fe).Hp, (fo if e[0] % 2 else fe).Wp), generator=g) * 1.2 - 0.1).to(dev)
                 for e in elements]
        frames = {0: fe, 1: fo}

        def eight():
            return [I.finish(p, S, idx, frames[e[0] % 2], metres=True) for p, e in zip(preds, elements)]

        ts, iters = alternate({"mean": lambda: I.finish_mean(preds, S, idx, frames, elements, metres=True), "eight": eight}, 20)
        m = {k: statistics.median(v) for k, v in ts.items()}
        nbytes = n_scenes * H * W * 4 * 9
        say(f"finish   finish_mean, K = 8           1 launch  {spread(ts['mean'])}  {nbytes / (m['mean'] * 1e-6) / 1e9:8.1f} GB/s on "
            f"{nbytes / 1e6:.1f} MB (8 reads + 1 write per pixel)")
        say(f"finish   eight K13 finish             8 launches {spread(ts['eight'])}  (8 reads + 8 writes; no inverse, no mean)")
        say(f"finish   {iters} calls per window; eight finish / finish_mean = x{m['eight'] / m['mean']:.2f}")
        del preds, groups
        if not args.no_model:
            from jspsr_amd.JSPSR import Model
            torch.manual_seed(0)
            model = Model(dict(IC, COP30=1), num_feature=32).to(dev).eval()
            model.compute_dtype = torch.bfloat16
            span, lo = np.float32(P["elev_max"] - P["elev_min"]), np.float32(P["elev_min"])
            base = np.array([np.float32(b) for b in S.base], dtype=np.float32)

            def ours():
                return list(I.predict_scenes(model, S, batch_size=8, pad=pad, tta="d4").rasters().values())

            def by_hand():
                acc = None
                for e in elements:
                    St = I.InferenceScenes(**{k: [np.ascontiguousarray(I.d4_apply(s[k], e)) for s in scenes] for k in KINDS},
                                           device=dev, base=list(S.base), **P)
                    y = I.predict_scenes(model, St, batch_size=8, pad=pad, metres=False).rasters()
                    y = np.stack([I.d4_invert(v, e) for v in y.values()])
                    acc = y if acc is None else acc + y
                mean = np.clip(acc / np.float32(len(elements)), 0.0, 1.0)
                return list(np.exp(mean * np.log(span)) + lo + base[:, None, None])

            a, b = ours(), by_hand()
            for _ in range(2):
                ours()
                by_hand()
            diff = max(float(np.abs(x - y).max()) for x, y in zip(a, b))
            ts = {"ours": [], "hand": []}
            for _ in range(args.reps):
                for name, fn in (("ours", ours), ("hand", by_hand)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            m = {k: statistics.median(v) for k, v in ts.items()}
            say(f"end to end (JSPSR image + mask, 32 features, bf16, forwards of at most 8 samples; ms per pass, host clock, final copy included)")
            say(f"end to end predict_scenes(tta='d4') + rasters()                         {spread(ts['ours'], 'ms')}")
            say(f"end to end 8 x (numpy transform, upload, predict_scenes, rasters), numpy mean {spread(ts['hand'], 'ms')}")
            say(f"end to end by hand / tta = x{m['hand'] / m['ours']:.2f}; {n_scenes * H * W / (m['ours'] * 1e-3) / 1e6:.1f} Mpixel/s of scene "
                f"pixels with tta; max |difference| of the two results {diff:.3e} m (numpy's exp and log against the device's; where the two legs' forwards differ in batch size, bf16 rounding too: one bf16 ulp of the network's output near 0.8 is 8 m under elev_log)")
            del model
        del S
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
