"""K17 (voids in whole-scene inference, csrc/scene_voids.hip) on one MI355X.

  kernels     on one SIDE x SIDE scene (default 4096) and three void patterns -- 1 % speckle, disks of radius 200, a "coast"
              (a half plane with a wavy edge, about 50 % void) --: `infer.nearest_seed` of the valid pixels (the fill's
              transform, no limit), `infer.fill_voids`, and the margin pass (`nearest_seed` of the voids with limit 16 and
              the threshold into the uint8 plane).  Device events around `iters` calls, warmed up; median, min and max of
              the repetitions in ms.  d2 is compared with scipy's exact EDT where scipy imports.
  host route  what the feature replaces, in the same run: `scipy.ndimage.distance_transform_edt(return_indices=True)` on the
              void mask and the numpy gather, a host clock; "host baseline not measured" where scipy does not import.
  store       the whole `InferenceScenes` construction (lr_dem alone) with `nodata` (void_margin 16) and, on the scene filled
              by hand, without: a host clock around the constructor and a synchronise.
  predict     `predict_scenes(tile=512, overlap=64, trim=16, batch_size=8)`, JSPSR image + mask, 32 features, fp32, on a
              2048 x 2048 scene (the tiled case of tools/bench_tiled_infer.py) with disks of voids and without; and the one
              `mask_out` launch of that call by device events.
Reported, not gated.
Usage: python tools/bench_void_fill.py [--side N] [--reps R] [--no-model] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True)
NODATA = -32767.0
MARGIN = 16


def spread(xs, unit="ms"):
    return f"median {statistics.median(xs):10.3f}  min {min(xs):10.3f}  max {max(xs):10.3f} {unit} (n={len(xs)})"


def patterns(np, n):
    """name -> (n, n) bool void mask."""
    rs = np.random.RandomState(17)
    yy, xx = np.mgrid[0:n, 0:n]
    speckle = rs.rand(n, n) < 0.01
    disks = np.zeros((n, n), bool)
    for cy, cx in rs.randint(0, n, (max(1, n * n // (1024 * 1024)), 2)):          # one disk per Mpixel
        disks |= (yy - cy) ** 2 + (xx - cx) ** 2 <= 200 ** 2
    coast = yy > n // 2 + (n / 16) * np.sin(xx / (n / 40.0)) + (n / 64) * np.sin(xx / (n / 300.0))
    return {"speckle 1 %": speckle, "disks r=200": disks, "coast": coast}


def dem_of(np, n):
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    return (250 + 60 * np.sin(yy / 70) * np.cos(xx / 90) + 0.01 * yy + 0.005 * xx).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import infer as I
    assert torch.cuda.is_available(), "bench_void_fill needs the MI355X"
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def timed(fn, reps):
        fn()
        fn()                                                                       # warm
        torch.cuda.synchronize()
        iters = max(1, min(50, int(0.2 / max(events(fn, 1) * 1e-3, 1e-6))))          # about 0.2 s per timed window
        return [events(fn, iters) for _ in range(reps)], iters

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    n = args.side
    say(f"# K17, voids in whole-scene inference; {torch.cuda.get_device_name(0)}; one {n} x {n} scene ({n * n / 1e6:.1f} Mpixel)")
    dem = dem_of(np, n)
    table = torch.tensor([[0, n, n]], dtype=torch.int64, device=dev)
    base = torch.tensor([float(dem.min())], dtype=torch.float32, device=dev)
    for name, void in patterns(np, n).items():
        say()
        say(f"# {name}: {void.mean() * 100:.2f} % void")
        raw = dem.copy()
        raw[void] = NODATA
        v = torch.from_numpy(void.astype(np.uint8).reshape(-1)).to(dev)
        valid = v ^ 1
        store = torch.from_numpy(raw.reshape(-1)).to(dev)
        src, d2 = I.nearest_seed(valid, table)
        t, iters = timed(lambda: I.nearest_seed(valid, table), args.reps)
        say(f"nearest_seed (valid pixels, no limit)   {spread(t)}  {n * n / statistics.median(t) / 1e3:8.1f} Mpixel/s  ({iters} calls per window)")
        t, iters = timed(lambda: I.fill_voids(store, v, src, table, base), args.reps)
        say(f"fill_voids                              {spread(t)}  ({iters} calls per window)")
        t, iters = timed(lambda: (I.nearest_seed(v, table, MARGIN)[1] >= 0).to(torch.uint8), args.reps)
        say(f"margin pass (voids, limit {MARGIN}) + threshold {spread(t)}  ({iters} calls per window)")
        if ndimage is None:
            say("host baseline not measured (scipy does not import here)")
        else:
            def host():
                dist, idx = ndimage.distance_transform_edt(void, return_indices=True)
                out = raw[idx[0], idx[1]]
                return dist, out
            ts = []
            for _ in range(2):
                t0 = time.perf_counter()
                dist, out = host()
                ts.append((time.perf_counter() - t0) * 1e3)
            say(f"host route: scipy EDT with indices + numpy gather  {spread(ts)}")
            same = np.array_equal(np.rint(dist ** 2).astype(np.int64), d2.cpu().numpy().reshape(n, n).astype(np.int64))
            say(f"d2 equals scipy's squared EDT everywhere: {same}")
            del dist, out

        def with_nodata():
            return I.InferenceScenes([raw[..., None]], device=dev, nodata=NODATA, void_margin=MARGIN, **P)

        filled = store.cpu().numpy().reshape(n, n, 1)
        S = with_nodata()
        assert np.array_equal(S.store["lr_dem"].cpu().numpy(), filled.reshape(-1))
        ref_base = [S.base[0]]
        del S

        def without():
            return I.InferenceScenes([filled], device=dev, base=ref_base, **P)

        t_with, t_without = [], []
        for _ in range(max(2, args.reps // 2)):
            t_with.append(clock(with_nodata)[0])
            t_without.append(clock(without)[0])
        say(f"InferenceScenes(nodata=..., void_margin={MARGIN})  {spread(t_with)}")
        say(f"InferenceScenes of the filled scene, no nodata   {spread(t_without)}")
        del src, d2, store, v, valid
        torch.cuda.empty_cache()
    if not args.no_model:
        from jspsr_amd.JSPSR import Model
        from tests import batches_ref as R
        IC, KINDS = {"lr_dem": 1, "image": 3, "mask": 15}, ("lr_dem", "image", "mask")
        torch.manual_seed(0)
        model = Model(dict(IC, COP30=1), num_feature=32).to(dev).eval()
        h = w = 2048
        small = R.make_scenes([(512, 512)], seed=1)[0]                                # the scene of tools/bench_tiled_infer.py
        scene = {k: np.ascontiguousarray(np.tile(small[k], (h // 512, w // 512, 1))) for k in KINDS}
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        scene["lr_dem"] = (scene["lr_dem"] + (0.01 * yy + 0.005 * xx)[..., None]).astype(np.float32)
        void = patterns(np, h)["disks r=200"]
        holed = dict(scene, lr_dem=scene["lr_dem"].copy())
        holed["lr_dem"][void] = NODATA
        PM = dict(P, scale_mask=True)
        plain = I.InferenceScenes(**{k: [scene[k]] for k in KINDS}, device=dev, **PM)
        voids = I.InferenceScenes(**{k: [holed[k]] for k in KINDS}, device=dev, nodata=NODATA, void_margin=MARGIN, **PM)
        kw = dict(batch_size=8, tile=512, overlap=64, trim=16)
        say()
        say(f"# predict_scenes on {h} x {w}, tile 512, overlap 64, trim 16, batch 8, JSPSR nf-32 fp32; disks: {void.mean() * 100:.2f} % void, "
            f"void_out {float(voids.void_out.float().mean()) * 100:.2f} %")
        legs = {"no voids in the store": lambda: I.predict_scenes(model, plain, **kw),
                "voids, mask_voids=True": lambda: I.predict_scenes(model, voids, **kw),
                "voids, mask_voids=False": lambda: I.predict_scenes(model, voids, mask_voids=False, **kw)}
        for one in legs.values():
            one()
        ts = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, one in legs.items():                                                # the legs alternate within a repetition
                ts[k].append(clock(one)[0])
        for k in legs:
            say(f"{k:26s} {spread(ts[k])}")
        r = legs["voids, mask_voids=False"]()
        rows = I._mask_rows(voids, [0], r.offsets)
        t, iters = timed(lambda: I.mask_out(r.buffer, voids.void_out, rows, NODATA), args.reps)
        say(f"mask_out alone, one launch  {spread(t)}  ({iters} calls per window)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
