"""K26 (exact area downsample of HWC uint8 rasters, csrc/area.hip) on one MI355X.

  kernel      `resample.area_rasters`, four cases: one 16384 x 16384 x 3 image -> 4096 x 4096 (ratio 4) and -> 4369 x 4369
              (ratio 3.75), one 8192 x 8192 x 15 mask -> 2048 x 2048 under "majority", and eight 1336 x 1336 x 3 -> 334 x 334
              scenes in ONE launch.  Device events around `iters` calls, warmed up; median, min and max of the repetitions in
              microseconds per call, and the bytes read over that time beside the HBM read rate (6.29 TB/s measured, float4 copy,
              MI355X): the pass has to read every source byte once.  A source smaller than the 256 MiB Infinity Cache is copied
              until the copies pass 512 MB and the calls rotate through them.
  torch       where the ratio is a whole number: permute -> float -> F.avg_pool2d -> + 0.5, floor -> uint8 -> permute on the same
              device, timed the same way in the same run, the two alternating; its output is compared with the kernel's.
  host route  what the feature replaces, for the whole-number ratios: the block sum in numpy rounded half up in integers (the
              restatement at such a ratio) plus the upload of the result, a host clock around both and a synchronise.
  store       the construction of an `InferenceScenes` of one 4096 x 4096 scene with its image at 16384 x 16384 and
              guide_resample="area", and from the host-resampled image without: a host clock around the constructor and a
              synchronise; the host's resampling time is listed on its own.
  kernel times  come from a trace in a run of its own: `rocprofv3 --kernel-trace --stats -d DIR -o area --output-format csv --
              python tools/bench_area.py --trace-loop` runs each case 20 times and nothing else; `tools/ktrace.py` reads it.
Reported, not gated.
Usage: python tools/bench_area.py [--reps R] [--iters N] [--out FILE] [--trace-loop] [--no-store]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_READ = 6.29e12                     # bytes / s, measured float4 copy rate
CACHE = 256 << 20


def spread(xs, unit="us"):
    return f"median {statistics.median(xs):10.2f}  min {min(xs):10.2f}  max {max(xs):10.2f} {unit} (n={len(xs)})"


def block_mean(a, r):
    """The restatement where both ratios are the whole number r: the block sum, rounded half up in integers."""
    import numpy as np
    h, w, c = a.shape
    s = a.reshape(h // r, r, w // r, r, c).sum(axis=(1, 3), dtype=np.uint32)
    return ((s + (r * r) // 2) // (r * r)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-loop", action="store_true", help="only run each case 20 times, for rocprofv3 --kernel-trace")
    ap.add_argument("--no-store", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from jspsr_amd import infer as I
    from jspsr_amd import resample as RS
    assert torch.cuda.is_available(), "bench_area needs the MI355X"
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, iters):
        """microseconds per call by device events around `iters` calls."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(iters):
            fn(k)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1000.0 / iters

    say(f"# K26, exact area downsample of uint8 rasters; {torch.cuda.get_device_name(0)}; {args.iters} calls per window, {args.reps} windows")
    g = torch.Generator(device=dev).manual_seed(26)
    cases = (("one 16384^2 x 3 image -> 4096^2 (ratio 4)", 1, (16384, 16384), (4096, 4096), 3, "area"),
             ("the same image -> 4369^2 (ratio 3.75)", 1, (16384, 16384), (4369, 4369), 3, "area"),
             ("one 8192^2 x 15 mask -> 2048^2, majority", 1, (8192, 8192), (2048, 2048), 15, "majority"),
             ("eight 1336^2 x 3 scenes -> 334^2, one launch", 8, (1336, 1336), (334, 334), 3, "area"))
    for name, count, (h, w), (H, W), C, mode in cases:
        nbytes = count * h * w * C
        copies = 1 if nbytes > CACHE else -(-(512 << 20) // nbytes)
        if mode == "majority":
            one = (torch.randint(0, C + 3, (count * h * w, 1), device=dev, generator=g) == torch.arange(C, device=dev)).to(torch.uint8).view(-1)
        else:
            one = torch.randint(0, 256, (nbytes,), device=dev, generator=g, dtype=torch.uint8)
        bufs = [one] + [one.clone() for _ in range(copies - 1)]
        table = [(k * h * w, h, w) for k in range(count)]
        shapes = [(H, W)] * count
        ours = lambda k: RS.area_rasters(bufs[k % copies], table, C, shapes, mode)
        whole = h % H == 0 and w % W == 0 and h // H == w // W and mode == "area"
        r = h // H

        def theirs(k):
            x = bufs[k % copies].view(count, h, w, C).permute(0, 3, 1, 2).float()
            return torch.floor(F.avg_pool2d(x, r) + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

        for k in range(3):
            ours(k)
            if whole:
                theirs(k)
        torch.cuda.synchronize()
        if args.trace_loop:
            for k in range(20):
                ours(k)
                if whole:
                    theirs(k)
            torch.cuda.synchronize()
            del bufs, one
            continue
        t_ours, t_torch = [], []
        for _ in range(args.reps):                                                # alternating windows
            t_ours.append(timed(ours, args.iters))
            if whole:
                t_torch.append(timed(theirs, max(2, args.iters // 4)))
        rate = nbytes / (statistics.median(t_ours) * 1e-6)
        say()
        say(f"# {name}: {nbytes / 1e6:.1f} MB read, {count * H * W * C / 1e6:.1f} MB written, {copies} rotating source buffer(s)")
        say(f"area_rasters (K26)                {spread(t_ours)}  {rate / 1e12:6.3f} TB/s read = {100 * rate / HBM_READ:5.1f} % of the HBM read rate")
        if whole:
            say(f"torch float avg_pool2d route      {spread(t_torch)}  {nbytes / (statistics.median(t_torch) * 1e-6) / 1e12:6.3f} TB/s read")
            same = torch.equal(ours(0)[0].view(count, H, W, C), theirs(0))
            say(f"the two outputs are {'equal' if same else 'NOT equal'} byte for byte")
            host = one.cpu().numpy().reshape(count, h, w, C)
            t_host, t_mean = [], []
            for _ in range(2):
                t0 = time.perf_counter()
                small = np.stack([block_mean(a, r) for a in host])
                t1 = time.perf_counter()
                up = torch.from_numpy(small).to(dev)
                torch.cuda.synchronize()
                t_host.append((time.perf_counter() - t0) * 1e3)
                t_mean.append((t1 - t0) * 1e3)
            say(f"host route: numpy block mean in integers + upload  {spread(t_host, 'ms')}, of it the block mean {statistics.median(t_mean):.1f} ms")
            say(f"the host's result is {'equal' if torch.equal(up.view(-1), ours(0)[0]) else 'NOT equal'} to the kernel's")
            del host, up
        del bufs, one
        torch.cuda.empty_cache()

    if args.trace_loop or args.no_store:
        if args.out and not args.trace_loop:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    # the store: one 4096 x 4096 scene whose image is held at 16384 x 16384
    P = dict(relative=True, elev_min=-80, elev_max=2000, elev_log=True)
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:4096, 0:4096].astype(np.float32)
    lr = (1500 + 15 * np.sin(yy / 7) * np.cos(xx / 9) + rs.uniform(0, 5, (4096, 4096))).astype(np.float32)[..., None]
    fine = np.random.default_rng(6).integers(0, 256, (16384, 16384, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    small = block_mean(fine, 4)
    t_host = (time.perf_counter() - t0) * 1e3
    t_with, t_without = [], []
    for rep in range(3):
        for which, ts in (("with", t_with), ("without", t_without)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if which == "with":
                S = I.InferenceScenes(lr_dem=[lr], image=[fine], guide_resample="area", device=dev, **P)
            else:
                S = I.InferenceScenes(lr_dem=[lr], image=[small], device=dev, **P)
            torch.cuda.synchronize()
            if rep:                                                               # the first round warms both up
                ts.append((time.perf_counter() - t0) * 1e3)
            if which == "with":
                same = torch.equal(S.store["image"].cpu(), torch.from_numpy(small).view(-1))
            del S
    say()
    say("# InferenceScenes of one 4096 x 4096 scene (lr_dem and image), host clock around the constructor and a synchronise")
    say(f"image 16384 x 16384 x 3 + guide_resample='area' ({fine.nbytes / 1e6:.1f} MB uploaded)   {spread(t_with, 'ms')}")
    say(f"image 4096 x 4096 x 3 resampled on the host ({small.nbytes / 1e6:.1f} MB uploaded)      {spread(t_without, 'ms')}")
    say(f"the host's own block mean for that image, not in the line above: {t_host:.1f} ms (once); the stores' images are "
        f"{'equal' if same else 'NOT equal'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
