"""K25 (rasters resampled to a finer grid, csrc/resample.hip) on one MI355X.

  kernel      `resample.resample_rasters`, bicubic, two cases: one 1024 x 1024 -> 3840 x 3840 raster, and eight 89 x 89 ->
              334 x 334 rasters in ONE launch (the dataset's scene at the 3.75 ratio).  Device events around `iters` calls,
              warmed up; median, min and max of the repetitions in microseconds per call, and the share of the HBM write rate
              (6.29 TB/s measured, MI355X) at the 4 bytes per output pixel the pass has to write.
  torch       `torch.nn.functional.interpolate(mode="bicubic", align_corners=False)` on the same device, timed the same way in
              the same run, the two alternating; for the eight rasters that is eight calls (torch batches equal shapes only
              through a stacked tensor, which a flat store of scenes is not).  The largest difference between the outputs is
              printed beside the times.
  host route  what the feature replaces: F.interpolate on the CPU plus the upload, a host clock around both and a synchronise.
  store       the construction of an `InferenceScenes` of one 4096 x 4096 scene: from a 1093 x 1093 lr_dem with
              lr_resample="bicubic" (4.8 MB uploaded), and from the host-resampled 4096 x 4096 raster without (67 MB): a host
              clock around the constructor and a synchronise; the host's resampling time is listed on its own.
  kernel times  come from a trace in a run of its own: `rocprofv3 --kernel-trace --stats -d DIR -o rs --output-format csv --
              python tools/bench_resample.py --trace-loop` runs each case 50 times and nothing else; `tools/ktrace.py` reads it.
Reported, not gated.
Usage: python tools/bench_resample.py [--reps R] [--iters N] [--out FILE] [--trace-loop]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_WRITE = 6.29e12                    # bytes / s, measured float4 copy rate


def spread(xs, unit="us"):
    return f"median {statistics.median(xs):10.2f}  min {min(xs):10.2f}  max {max(xs):10.2f} {unit} (n={len(xs)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-loop", action="store_true", help="only run each case 50 times, for rocprofv3 --kernel-trace")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from jspsr_amd import infer as I
    from jspsr_amd import resample as RS
    assert torch.cuda.is_available(), "bench_resample needs the MI355X"
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, iters):
        """microseconds per call by device events around `iters` calls."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1000.0 / iters

    def dem(h, w, seed):
        rs = np.random.RandomState(seed)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        return (1500 + 15 * np.sin(yy / 7) * np.cos(xx / 9) + rs.uniform(0, 5, (h, w))).astype(np.float32)

    say(f"# K25, bicubic resample to a finer grid; {torch.cuda.get_device_name(0)}; {args.iters} calls per window, {args.reps} windows")
    for name, count, (h, w), (H, W) in (("one 1024^2 -> 3840^2 raster", 1, (1024, 1024), (3840, 3840)),
                                        ("eight 89^2 -> 334^2 rasters, one launch", 8, (89, 89), (334, 334))):
        host = [dem(h, w, s) for s in range(count)]
        flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in host])).to(dev)
        table = [(k * h * w, h, w) for k in range(count)]
        shapes = [(H, W)] * count
        planes = [flat[k * h * w:(k + 1) * h * w].view(1, 1, h, w) for k in range(count)]
        ours = lambda: RS.resample_rasters(flat, table, shapes)
        theirs = lambda: [F.interpolate(p, size=(H, W), mode="bicubic", align_corners=False) for p in planes]
        for _ in range(20):                                                       # warm up both, tables uploaded
            ours(), theirs()
        torch.cuda.synchronize()
        if args.trace_loop:                                                       # kernel times come from the profiler's trace
            for _ in range(50):
                ours(), theirs()
            torch.cuda.synchronize()
            continue
        t_ours, t_torch = [], []
        for _ in range(args.reps):                                                # alternating windows
            t_ours.append(timed(ours, args.iters))
            t_torch.append(timed(theirs, args.iters))
        out_bytes = 4.0 * count * H * W
        got = ours()[0].view(count, H, W)
        ref = torch.cat(theirs()).view(count, H, W)
        ref64 = torch.stack([F.interpolate(torch.from_numpy(a.astype(np.float64))[None, None], size=(H, W), mode="bicubic",
                                           align_corners=False)[0, 0] for a in host[:1]])
        say()
        say(f"# {name}: {out_bytes / 1e6:.1f} MB written, {4.0 * count * h * w / 1e6:.2f} MB read")
        say(f"resample_rasters (K25)            {spread(t_ours)}  {out_bytes / (statistics.median(t_ours) * 1e-6) / 1e12:6.3f} TB/s written = "
            f"{100 * out_bytes / (statistics.median(t_ours) * 1e-6) / HBM_WRITE:5.1f} % of the HBM write rate")
        say(f"F.interpolate on the device x{count}     {spread(t_torch)}  {out_bytes / (statistics.median(t_torch) * 1e-6) / 1e12:6.3f} TB/s written")
        say(f"max |K25 - torch fp32 on the device| = {float((got - ref).abs().max()):.3e} m;  against fp64 on the CPU (first raster): "
            f"K25 {float((got[0].cpu().double() - ref64[0]).abs().max()):.3e} m, torch fp32 {float((ref[0].cpu().double() - ref64[0]).abs().max()):.3e} m")
        t_host = []
        for _ in range(3):
            t0 = time.perf_counter()
            up = [F.interpolate(torch.from_numpy(a)[None, None], size=(H, W), mode="bicubic", align_corners=False).to(dev) for a in host]
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) * 1e6)
            del up
        say(f"host route: F.interpolate on the CPU ({torch.get_num_threads()} threads) + upload  {spread(t_host)}")

    if args.trace_loop:
        return
    # the store: one 4096 x 4096 scene from a 1093 x 1093 lr_dem
    P = dict(relative=True, elev_min=-80, elev_max=2000, elev_log=True)
    coarse = dem(1093, 1093, 99)
    t0 = time.perf_counter()
    fine = F.interpolate(torch.from_numpy(coarse)[None, None], size=(4096, 4096), mode="bicubic", align_corners=False)[0, 0]
    fine = fine.clamp(float(coarse.min()), float(coarse.max())).numpy()
    t_resample_host = (time.perf_counter() - t0) * 1e3
    t_with, t_without = [], []
    for rep in range(4):
        for which, ts in (("with", t_with), ("without", t_without)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if which == "with":
                S = I.InferenceScenes(lr_dem=[coarse[..., None]], lr_resample="bicubic", lr_shape=(4096, 4096), device=dev, **P)
            else:
                S = I.InferenceScenes(lr_dem=[fine[..., None]], base=[coarse.min()], device=dev, **P)
            torch.cuda.synchronize()
            if rep:                                                               # the first round warms both up
                ts.append((time.perf_counter() - t0) * 1e3)
            del S
    say()
    say("# InferenceScenes of one 4096 x 4096 scene (lr_dem alone), host clock around the constructor and a synchronise")
    say(f"lr_dem 1093 x 1093 + lr_resample='bicubic' ({coarse.nbytes / 1e6:.1f} MB uploaded)   {spread(t_with, 'ms')}")
    say(f"lr_dem 4096 x 4096 resampled on the host ({fine.nbytes / 1e6:.1f} MB uploaded)       {spread(t_without, 'ms')}")
    say(f"the host's own F.interpolate + clamp for that raster, not in the line above: {t_resample_host:.1f} ms (once)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
