"""K13 (whole-scene inference, jspsr_amd/infer.py) on one MI355X.

  launches    `infer.prepare` and `infer.finish` (one launch each) against the same work done with the calls the package
              offered before: per scene `metrics.scale_data` (jspsr_elev_scale_f32), `tiles.scale_image`, `tiles.scale_mask`
              on the uploaded HWC rasters turned to CHW, one `tiles.add_padding` per raster, a stack per kind; and
              `tiles.remove_padding`, clamp, `metrics.descale_data`, `+ base`.  Device events around windows of at least 0.1 s
              of K13's calls, warmed up, the two legs alternating within a repetition; median, min and max of the repetitions.
              ACCEPTANCE: K13's median + its own max - min spread < the composition's median, for both launches.
              Achieved bytes/s on the algorithmic count -- prepare writes 76 B per frame pixel (19 fp32 planes) and reads
              22 B per source pixel (fp32 + 3 + 15 bytes); finish moves 8 B per pixel -- as a share of the 6.29 TB/s the
              float4 copy reaches on this chip.  Reported, not gated.  The composition's launches are counted from its
              code: per scene 2 (DEM) + 4 (image: contiguous CHW, float, / 255, pad) + 4 (mask), and a stack per kind.
  workload 1  8 scenes of 334 x 334, pad 89 (cal_pad: a 512 x 512 frame), image + mask
  workload 2  one 4096 x 4096 scene, pad 0, image + mask
  end to end  `predict_scenes`, Mpixel/s of scene pixels, a host clock around passes that end in a synchronise.  Workload 1
              with JSPSR image + mask, 32 features, bf16, one batch of 8.  Workload 2 with a pass-through model (it returns
              its DEM input, no launch): the pass's own cost at that size, two launches and the host code around them.
              A real forward of one 4096 x 4096 frame is NOT run: no convolution kernel is tested beyond a 768 x 4096
              strip, and scenes too large for one forward go through tiling.py, which takes prepare's pad-0 output.
Usage: python tools/bench_infer.py [--reps R] [--workloads 1,2] [--no-model] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True, scale_mask=True)
IC = {"lr_dem": 1, "image": 3, "mask": 15}
COPY_RATE = 6.29e12
WINDOW = 0.1                # seconds of K13's calls in one timed window


def spread(xs):
    return f"median {statistics.median(xs):10.1f}  min {min(xs):10.1f}  max {max(xs):10.1f} us (n={len(xs)})"


def events(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


class PassThrough:
    """Stands in for a model where no forward is run: takes JSPSR's inputs, returns the DEM plane it was given."""
    size_multiple = 8

    def eval(self):
        return self

    def __call__(self, dem, *others):
        return dem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--workloads", default="1,2")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import infer as I, metrics as M, tiles as T
    from tests import batches_ref as R
    assert torch.cuda.is_available(), "bench_infer needs the MI355X"
    dev = "cuda:0"
    lines, ok = [], True

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# K13, whole-scene inference; {torch.cuda.get_device_name(0)}")
    for wl in [int(w) for w in args.workloads.split(",")]:
        n_scenes, side, pad, floor_iters = ((8, 334, 89, 200), (1, 4096, 0, 10))[wl - 1]
        scenes = R.make_scenes([(side, side)] * n_scenes, seed=wl, coord=False)
        S = I.InferenceScenes(**{k: [s[k] for s in scenes] for k in ("lr_dem", "image", "mask")}, device=dev, **P)
        idx = list(range(n_scenes))
        inputs, fr = I.prepare(S, idx, pad, 8)
        raw = {k: [torch.from_numpy(s[k]).to(dev) for s in scenes] for k in ("lr_dem", "image", "mask")}      # HWC, as decoded
        base = [float(np.float32(b)) for b in S.base]
        base_t = torch.tensor(base, dtype=torch.float32, device=dev)[:, None, None, None]

        def composed_prepare():
            dem, img, msk = [], [], []
            for i in range(n_scenes):
                z = M.scale_data(raw["lr_dem"][i].permute(2, 0, 1), P["elev_min"], P["elev_max"], True, base_elev=base[i])
                dem.append(T.add_padding(z, pad))
                img.append(T.add_padding(T.scale_image(raw["image"][i].permute(2, 0, 1).contiguous()), pad))
                msk.append(T.add_padding(T.scale_mask(raw["mask"][i].permute(2, 0, 1).contiguous(), 15), pad))
            if n_scenes == 1:
                return [dem[0][None], img[0][None], msk[0][None]]
            return [torch.stack(dem), torch.stack(img), torch.stack(msk)]

        pred = (torch.rand((n_scenes, 1, fr.Hp, fr.Wp), generator=torch.Generator().manual_seed(2)) * 1.2 - 0.1).to(dev)

        def composed_finish():
            w = T.remove_padding(pred, pad).clamp(0.0, 1.0)
            return M.descale_data(w, P["elev_min"], P["elev_max"], True) + base_t

        # the two ways give the same numbers (the DEM through two logf paths: 1 ulp of the scaled value)
        for a, b in zip(inputs, composed_prepare()):
            assert a.shape == b.shape and float((a - b).abs().max()) <= 2e-7, float((a - b).abs().max())
        assert torch.equal(I.finish(pred, S, idx, fr), composed_finish()[:, 0])
        n_launch = n_scenes * 10 + (3 if n_scenes > 1 else 0)
        legs = {"prepare": (lambda: I.prepare(S, idx, pad, 8), composed_prepare, n_launch,
                            n_scenes * (fr.Hp * fr.Wp * 76 + side * side * 22)),
                "finish": (lambda: I.finish(pred, S, idx, fr), composed_finish, 4, n_scenes * side * side * 8)}
        say()
        say(f"# workload {wl}: {n_scenes} scene(s) of {side} x {side}, pad {pad} -> frame {fr.Hp} x {fr.Wp}, image + mask; "
            f"us per call, device events around windows of at least {WINDOW} s of K13's calls, legs alternate within a repetition")
        for name, (new, old, launches, nbytes) in legs.items():
            for _ in range(3):
                new()
                old()
            # a window of a few ms measures one hiccup of the host as much as the calls: size it to WINDOW seconds of K13's
            # calls (the composition's window is longer), after one untimed window of each leg
            iters = max(floor_iters, int(WINDOW / (events(torch, new, floor_iters) * 1e-6)))
            events(torch, old, floor_iters)
            t_new, t_old = [], []
            for _ in range(args.reps):
                t_new.append(events(torch, new, iters))
                t_old.append(events(torch, old, iters))
            m_new, m_old = statistics.median(t_new), statistics.median(t_old)
            rate = nbytes / (m_new * 1e-6)
            good = m_new + (max(t_new) - min(t_new)) < m_old
            ok = ok and good
            say(f"{name:8s} K13         1 launch    {spread(t_new)}  {rate / 1e9:8.1f} GB/s on {nbytes / 1e6:.1f} MB = "
                f"{100 * rate / COPY_RATE:.1f} % of the float4-copy rate")
            say(f"{name:8s} composition {launches:2d} launches {spread(t_old)}  {nbytes / (m_old * 1e-6) / 1e9:8.1f} GB/s")
            say(f"{name:8s} {iters} calls per window; K13 " + " ".join(f"{t:.1f}" for t in t_new) + "; composition " +
                " ".join(f"{t:.1f}" for t in t_old))
            say(f"{name:8s} x{m_old / m_new:.2f}; ACCEPTANCE (K13 median + its spread < composition median): {'PASS' if good else 'FAIL'}")
        if not args.no_model:
            if wl == 1:
                from jspsr_amd.JSPSR import Model
                torch.manual_seed(0)
                model = Model(dict(IC, COP30=1), num_feature=32).to(dev).eval()
                model.compute_dtype = torch.bfloat16
                what = f"JSPSR image + mask, 32 features, bf16, one batch of {n_scenes}"
            else:
                model = PassThrough()
                what = "a pass-through model that returns its DEM input: prepare + finish + host code, NO network"
            one = lambda: I.predict_scenes(model, S, batch_size=n_scenes, pad=pad, model_name="jspsr")      # noqa: E731
            for _ in range(2):
                one()
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    r = one()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) / 3)
            px = n_scenes * side * side
            say(f"end to end predict_scenes ({what}): "
                f"{statistics.median(ts) * 1e3:.2f} ms per pass (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}) = "
                f"{px / statistics.median(ts) / 1e6:.1f} Mpixel/s of scene pixels; finite: {bool(torch.isfinite(r.buffer).all())}")
            del model, r
        del S, raw, inputs, pred
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
