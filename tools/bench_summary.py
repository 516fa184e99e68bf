"""K12 (the whole-set validation summary, jspsr_amd/summary.py) on one MI355X.

  yardstick   one 4096 x 4096 raster pair: `summary.scores_pooled` (K12(b), one candidate, one segment) against
              `metrics.tile_scores` (the one-tile kernel chain of csrc/metrics.hip: 12 histogram passes) on the same pair.
              Device events around `iters` calls, warmed up, legs alternating within a repetition; the median of the
              repetitions.  ACCEPTANCE: K12's median <= tile_scores' median + that leg's own max - min spread.
              Achieved bytes/s on the algorithmic count -- (n_cand + 1) reads + n_cand writes in the first pass, n_cand
              reads in each of the 7 select passes (3 for the e / |e| digits below the top one, which the first pass
              counts, 4 for |e - median|) -- as a share of 8 TB/s.  Reported, not gated.
  workload    114 scenes of 334 x 334, 9 tiles of 128, border 0.05 (the set of profiles/r06_eval_bench.txt): the
              assembly in one launch (`ScenePredictions.add`) against 114 x (clamp, de-scale, + base, `merge_tiles`); a
              4-candidate pooled + online `summarise` against the reference's way on the same box -- a device-to-host
              copy of the rasters, then the numpy lines of tests/summary_ref.py.  Ratios, no threshold; both must give
              the same numbers within the test tolerances (asserted).
  eval        `evaluate()`'s bf16 pass on that set with the collector unset (and, for information, set).  With
              --parent DIR (a built checkout of the parent commit) the unset pass is timed alternately in child processes
              of DIR and of this tree.
Usage: python tools/bench_summary.py [--legs yardstick,workload,eval] [--reps R] [--parent DIR] [--label TEXT] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True)
IC = {"lr_dem": 1, "image": 3, "mask": 15}
METRICS = {"PSNR": {"package": "piq"}, "RMSE": {"package": "local"}, "Median": {"package": "local"},
           "NMAD": {"package": "local"}, "LE95": {"package": "local"}}
LOSS = {"L1": 1, "L2": 1, "Grad": 0.1}
BORDER, N_SCENES, PEAK = 0.05, 114, 8e12


def spread(xs, unit=""):
    return f"median {statistics.median(xs):11.2f}  min {min(xs):11.2f}  max {max(xs):11.2f} {unit} (n={len(xs)}: " + \
        " ".join(f"{x:.1f}" for x in xs) + ")"


def events(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def eval_child(tree, passes):
    """Runs in a child process: `passes` timed bf16 evaluate() passes (collector unset) of the tree at `tree`."""
    sys.path.insert(0, tree)
    import torch
    from jspsr_amd import data as D, evaluate as EV, losses as L
    from jspsr_amd.JSPSR import Model
    from tests import batches_ref as R
    scenes = R.make_scenes([(334, 334)] * N_SCENES, seed=1)
    S = D.DeviceScenes(**{k: [s[k] for s in scenes] for k in ("lr_dem", "hr_dem", "image", "mask")}, device="cuda", scale_mask=True, **P)
    torch.manual_seed(0)
    model = Model(dict(IC, COP30=1), num_feature=32).to("cuda").eval()
    model.compute_dtype = torch.bfloat16

    def one():
        meter = EV.PerformanceMeter(METRICS, P["elev_min"], P["elev_max"], border=BORDER, elev_log=True)
        return EV.evaluate(model, D.TileCropBatches(S, 50, 128, 9), L.get_criterion(LOSS), meter, "JSPSR", IC)

    one()
    print("EVAL_CHILD " + json.dumps([timed(torch, one)[0] for _ in range(passes)]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="yardstick,workload,eval")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--label", default="working tree")
    ap.add_argument("--parent-label", default="parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--eval-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.eval_child:
        return eval_child(args.eval_child, args.reps)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import _lib, data as D, evaluate as EV, losses as L, metrics as M, summary as SM
    from tests import batches_ref as R, summary_ref as SR
    assert torch.cuda.is_available(), "bench_summary needs the MI355X"
    lib = _lib.load()
    legs = args.legs.split(",")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# K12, the whole-set validation summary; {torch.cuda.get_device_name(0)}; code: {args.label}")
    if "yardstick" in legs:
        say()
        say("# yardstick: one 4096 x 4096 pair, us per call, device events, legs alternate within a repetition")
        g = torch.Generator().manual_seed(1)
        n = 4096 * 4096
        gt01 = torch.rand(1, 1, 4096, 4096, generator=g) * 0.5 + 0.2
        pred01 = (gt01 + 0.004 * torch.randn(1, 1, 4096, 4096, generator=g)).clamp(0, 1).cuda()
        gt01 = gt01.cuda()
        pred_m, gt_m = (M.descale_data(t, P["elev_min"], P["elev_max"], False) for t in (pred01, gt01))   # the same pair in metres
        k12 = lambda: SM.scores_pooled(pred_m, gt_m, value_max=P["elev_max"])                               # noqa: E731
        old = lambda: M.tile_scores(pred01, gt01, P["elev_min"], P["elev_max"], 0.0, False)                  # noqa: E731
        for _ in range(3):
            k12()
            old()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.reps):
            a.append(events(torch, k12, 10))
            b.append(events(torch, old, 10))
        say(f"K12 scores_pooled (1 cand, 1 seg): {spread(a, 'us')}")
        say(f"metrics.tile_scores              : {spread(b, 'us')}")
        ma, mb, sb = statistics.median(a), statistics.median(b), max(b) - min(b)
        say(f"ACCEPTANCE K12 median {ma:.1f} <= tile_scores median {mb:.1f} + its spread {sb:.1f}: {'PASS' if ma <= mb + sb else 'FAIL'}"
            f"; ratio of medians (tile_scores / K12) {mb / ma:.2f}")
        passes = 7
        nbytes = 4 * n * ((1 + 1) + 1 + passes)
        say(f"K12 algorithmic bytes: (2 reads + 1 write) + {passes} select reads of {n} fp32 = {nbytes / 1e6:.1f} MB -> "
            f"{nbytes / (ma * 1e-6) / 1e12:.3f} TB/s = {nbytes / (ma * 1e-6) / PEAK:.3f} of 8 TB/s (whole call: 16 launches, the table upload and "
            "the host side of the call included)")
        r_new, r_old = k12()[0, 0].cpu().numpy(), old().cpu().numpy()
        say(f"K12 row (RMSE, Median, NMAD, LE95, PSNR): {[float(v) for v in r_new[:5]]}")
        say(f"tile_scores (PSNR on [0,1], RMSE, lower median, NMAD, kth LE95): {[float(v) for v in r_old]}")
        del pred01, gt01, pred_m, gt_m
    if "workload" in legs or "eval" in legs:
        scenes = R.make_scenes([(334, 334)] * N_SCENES, seed=1)
        S = D.DeviceScenes(**{k: [s[k] for s in scenes] for k in ("lr_dem", "hr_dem", "image", "mask")}, device="cuda", scale_mask=True, **P)
    if "workload" in legs:
        say()
        say(f"# workload: {N_SCENES} scenes of 334 x 334, 9 tiles of 128, border {BORDER}, log scaling")
        g = torch.Generator().manual_seed(2)
        gt_t = torch.cat([torch.from_numpy(S.scale_dem(s["hr_dem"][..., 0], S.base[i]))[None] for i, s in enumerate(scenes)])
        from jspsr_amd import tiles as T
        tiles = torch.cat([T.crop_tiles(gt_t[i:i + 1], 128, 9) for i in range(N_SCENES)])                  # the targets' tiles ...
        tiles = (tiles + 0.003 * torch.randn(tiles.shape, generator=g)).float().cuda()                      # ... plus noise: a good prediction
        c = SM.ScenePredictions(S, 128, 9, border=BORDER)
        bases = [torch.tensor(float(np.float32(b)), device="cuda") for b in S.base]

        def one_launch():
            c.reset()
            c.add(tiles)

        def per_scene():
            return [SM.compose_scene(tiles[9 * i:9 * i + 9], bases[i], 334, BORDER, P["elev_min"], P["elev_max"], True) for i in range(N_SCENES)]

        one_launch()
        ref = per_scene()
        torch.cuda.synchronize()
        n0 = lib.jspsr_launch_count(b"scenes_assemble")
        one_launch()
        assert lib.jspsr_launch_count(b"scenes_assemble") == n0 + 1
        assert torch.equal(c.buffer, torch.cat([r.reshape(-1) for r in ref])), "assembly differs from the composition"
        a, b = [], []
        for _ in range(args.reps):
            a.append(events(torch, one_launch, 20))
            b.append(events(torch, per_scene, 3))
        say("assembly, us per 114 scenes (device events); the two give the same bits")
        say(f"K12(a), one launch               : {spread(a, 'us')}")
        say(f"114 x (clamp, descale, +base, merge_tiles): {spread(b, 'us')}")
        say(f"ratio of medians (per scene / one launch): {statistics.median(b) / statistics.median(a):.1f}")
        rs = np.random.RandomState(3)
        fab = [s["lr_dem"][..., 0] + rs.uniform(-1, 1, (334, 334)).astype(np.float32) for s in scenes]
        fat = [s["lr_dem"][..., 0] * np.float32(0.999) + np.float32(0.7) for s in scenes]
        base_dev = {"COP30": "lr_dem", "FABDEM": SM.store_layout(S, fab), "FATHOM": SM.store_layout(S, fat)}
        kw = dict(value_max=P["elev_max"], border=BORDER, patch_size=128, online=True)
        dev_leg = lambda: SM.summarise(S, c, baselines=base_dev, **kw)                                      # noqa: E731

        def host_leg():
            rast = c.rasters()                                                                              # the device-to-host copy
            cands = {"SR": [rast[i] for i in S.ids], "COP30": [s["lr_dem"][..., 0] for s in scenes], "FABDEM": fab, "FATHOM": fat}
            return SR.summarise([s["hr_dem"][..., 0] for s in scenes], cands, int(128 * BORDER), P["elev_max"])

        dev_leg()
        a, b, got, want = [], [], None, None
        for r in range(args.reps):
            t, got = timed(torch, dev_leg)
            a.append(t)
            if r < args.host_reps:
                t, want = timed(torch, host_leg)
                b.append(t)
        n_px = N_SCENES * (334 - 2 * int(128 * BORDER)) ** 2
        say(f"summary of 4 candidates, pooled ({n_px} pixels) + online ({N_SCENES} scenes), ms per table, host clock to the result")
        say(f"summarise() on the device (one K12(b) call, one copy back): {spread(a, 'ms')}")
        say(f"copy to host + numpy (tests/summary_ref.py), {torch.get_num_threads()} torch threads / "
            f"{os.environ.get('OMP_NUM_THREADS', '?')} OMP: {spread(b, 'ms')}")
        say(f"ratio of medians (host / device): {statistics.median(b) / statistics.median(a):.1f}")
        worst = 0.0
        for name in got[0]:
            ref_row = want[0][name]
            SR.check_row(np.array([got[0][name][k] for k in SR.COLUMNS] + list(ref_row["brackets"])), ref_row, f"offline {name}")
            for i, sid in enumerate(S.ids):
                for k in ("RMSE", "NMAD", "LE95", "PSNR"):
                    worst = max(worst, float(SR.ulps(np.float32(got[2][name][sid][k]), want[2][name][i][k])))
                assert np.float32(got[2][name][sid]["Median"]) == want[2][name][i]["Median"]
        assert worst <= 2.0, worst
        say(f"both legs agree: offline rows within the test tolerances, online rows within {worst:.2f} fp32 ulp, medians bit-equal")
        say(f"offline table: { {n_: {k: round(v, 4) for k, v in row.items()} for n_, row in got[0].items()} }")
    if "eval" in legs:
        say()
        say("# evaluate(), bf16, nf 32 image + mask, 1026 tiles at batch 50: ms per pass, host clock to a device synchronise")
        from jspsr_amd.JSPSR import Model
        torch.manual_seed(0)
        model = Model(dict(IC, COP30=1), num_feature=32).to("cuda").eval()
        model.compute_dtype = torch.bfloat16
        c2 = SM.ScenePredictions(S, 128, 9, border=BORDER)

        def one(collector):
            c2.reset()
            meter = EV.PerformanceMeter(METRICS, P["elev_min"], P["elev_max"], border=BORDER, elev_log=True)
            return EV.evaluate(model, D.TileCropBatches(S, 50, 128, 9), L.get_criterion(LOSS), meter, "JSPSR", IC, collector=collector)

        one(None)
        one(c2)
        a, b = [], []
        for _ in range(args.reps):
            a.append(timed(torch, lambda: one(None))[0])
            b.append(timed(torch, lambda: one(c2))[0])
        say(f"this tree, collector unset : {spread(a, 'ms')}")
        say(f"this tree, collector set   : {spread(b, 'ms')}")
        del model
        torch.cuda.empty_cache()
        if args.parent:
            trees = {"parent": (os.path.abspath(args.parent), []), "this": (ROOT, [])}
            for _ in range(3):                                          # alternate fresh child processes: parent, this, parent, ...
                for key, (tree, acc) in trees.items():
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval-child", tree, "--reps", str(args.reps)],
                                         capture_output=True, text=True, timeout=600, cwd=tree)
                    row = [ln for ln in out.stdout.splitlines() if ln.startswith("EVAL_CHILD ")]
                    if out.returncode != 0 or not row:
                        raise RuntimeError(f"eval child of {tree} failed ({out.returncode}): {out.stderr[-2000:]}")
                    acc.extend(json.loads(row[0][len("EVAL_CHILD "):]))
            say(f"child processes, alternating (3 x {args.reps} passes each), collector unset:")
            say(f"{args.parent_label:28s}: {spread(trees['parent'][1], 'ms')}")
            say(f"{args.label:28s}: {spread(trees['this'][1], 'ms')}")
        else:
            say("parent commit in the same call: not measured (no --parent checkout given)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
