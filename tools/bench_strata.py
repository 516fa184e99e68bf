"""K22 (scores by terrain class, jspsr_amd/summary.py: stratified_rows / scores_by_class / slope_class_plane) on one MI355X.

Two pools: one 4096 x 4096 pair with one candidate, and 8 candidates of 2048 x 2048 against one ground truth.  n_classes in
{1, 4, 16} and 32, the most the entry takes; labels uniform over the classes, and with class 0 holding 90 %.
  stratified vs loop   `scores_by_class` (jspsr_strata_forward, one call of 16 launches) against the loop it replaces on the same
                       buffers: `scores_pooled(..., valid=(labels == c))` once per class (jspsr_summary_valid_forward, 16
                       launches and a full read of every candidate each).  The loop's masks are made ahead of the timed window,
                       which favours the loop.  Device events around `iters` calls, warmed up, the two legs alternating within a
                       repetition; median and spread of the repetitions.  The Median and the six brackets of every row must be
                       bit-equal between the legs (asserted).  The expectation to confirm or refute: the passes are
                       bandwidth-bound, so the stratified call is roughly flat in n_classes where the loop is linear in it,
                       and at n_classes = 1 it costs about one K18 call.
  stratified vs host   the host route: a device-to-host copy of the rasters and the labels, boolean indexing per class and
                       tests/summary_ref.py: scores.  Host clock to the result, the 4096 x 4096 pair with 4 uniform classes.
  slope_class_plane    one launch on the 4096 x 4096 scene against the bytes it must move: 4 B read and 1 B written per pixel.
Usage: python tools/bench_strata.py [--reps R] [--iters N] [--host-reps H] [--label TEXT] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMAX = 933.0
EXACT = [1, 5, 6, 7, 8, 9, 10]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--label", default="working tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import _lib, data as D, summary as SM
    from tests import summary_ref as SR
    assert torch.cuda.is_available(), "bench_strata needs the MI355X"
    lib = _lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def census():
        return lib.jspsr_launch_count(b"strata_prepare") + lib.jspsr_launch_count(b"strata_select")

    say(f"# K22, scores by terrain class; {torch.cuda.get_device_name(0)}; code: {args.label}")
    say(f"# us per call by device events around {args.iters} calls, legs alternating within a repetition; the loop's masks are made "
        "ahead of the timed window")
    g = torch.Generator().manual_seed(22)
    pools = []
    gt = (torch.rand(1, 4096, 4096, generator=g) * 500 + 100).cuda()
    pools.append(("one 4096 x 4096 pair, 1 candidate", [gt + 4.0 * torch.randn(1, 4096, 4096, generator=g).cuda()], gt))
    gt8 = (torch.rand(1, 2048, 2048, generator=g) * 500 + 100).cuda()
    pools.append(("8 candidates of 2048 x 2048", [gt8 + (0.5 + c) * torch.randn(1, 2048, 2048, generator=g).cuda() for c in range(8)], gt8))
    for title, cands, truth in pools:
        say()
        say(f"## {title}: {truth.numel()} pooled elements")
        ones = torch.ones_like(truth, dtype=torch.uint8)
        k18 = lambda: SM.scores_pooled(cands, truth, value_max=VMAX, valid=ones)                                        # noqa: E731
        for _ in range(3):
            k18()
        say(f"one K18 call, all-ones plane  : {spread([events(torch, k18, args.iters) for _ in range(args.reps)], 'us')}")
        for n_classes in (1, 4, 16, 32):
            for kind in ("uniform", "90 % in class 0"):
                if n_classes == 1 and kind != "uniform":
                    continue
                u = torch.rand(truth.shape, generator=g)
                if kind == "uniform":
                    labels = (u * n_classes).to(torch.uint8).clamp_(max=n_classes - 1)
                else:
                    labels = torch.where(u < 0.9, torch.zeros_like(u), 1 + (u - 0.9) * 10 * (n_classes - 1)).to(torch.uint8).clamp_(max=n_classes - 1)
                labels = labels.cuda()
                masks = [(labels == c).to(torch.uint8) for c in range(n_classes)]
                strat = lambda: SM.scores_by_class(cands, truth, labels, n_classes, value_max=VMAX)                      # noqa: E731
                loop = lambda: [SM.scores_pooled(cands, truth, value_max=VMAX, valid=m) for m in masks]                  # noqa: E731
                for _ in range(3):
                    strat()
                    loop()
                torch.cuda.synchronize()
                c0 = census()
                rows, counts = strat()
                assert census() == c0 + 16
                a, b = [], []
                for _ in range(args.reps):
                    a.append(events(torch, strat, args.iters))
                    b.append(events(torch, loop, args.iters))
                ma, mb = statistics.median(a), statistics.median(b)
                rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
                for c, (r, n) in enumerate(loop()):
                    assert int(n[0]) == int(counts[c])
                    assert rows[:, c][:, EXACT].tobytes() == r.cpu().numpy()[:, 0][:, EXACT].tobytes(), (n_classes, kind, c)
                say(f"### n_classes = {n_classes}, labels {kind} (largest class {int(counts.max())} of {truth.numel()})")
                say(f"stratified scores_by_class     : {spread(a, 'us')}")
                say(f"loop of scores_pooled(valid=)  : {spread(b, 'us')}")
                say(f"loop / stratified (medians): {mb / ma:.2f}; Median and brackets bit-equal between the legs, counts equal")
        if len(cands) == 1:
            n_classes = 4
            labels = (torch.rand(truth.shape, generator=g) * n_classes).to(torch.uint8).clamp_(max=n_classes - 1).cuda()

            def host_leg():
                p, t, lab = cands[0].cpu().numpy().reshape(-1), truth.cpu().numpy().reshape(-1), labels.cpu().numpy().reshape(-1)   # the copies
                e = p - t
                return [SR.scores(e[lab == c], VMAX) for c in range(n_classes)]

            def dev_leg():
                r, c = SM.scores_by_class(cands, truth, labels, n_classes, value_max=VMAX)
                return torch.cat((r.double().reshape(-1), c.double())).cpu().numpy()                                     # one copy back

            dev_leg()
            ta, tb, want, got = [], [], None, None
            for r in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = dev_leg()
                ta.append((time.perf_counter() - t0) * 1e3)
                if r < args.host_reps:
                    t0 = time.perf_counter()
                    want = host_leg()
                    tb.append((time.perf_counter() - t0) * 1e3)
            say("### the host route, 4 uniform classes")
            say(f"device call + one copy back, host clock to the result : {spread(ta, 'ms')}")
            say(f"copy to host + boolean indexing + summary_ref.scores per class, {torch.get_num_threads()} torch threads / "
                f"{os.environ.get('OMP_NUM_THREADS', '?')} OMP: {spread(tb, 'ms')}")
            say(f"host / device (medians): {statistics.median(tb) / statistics.median(ta):.1f}")
            for c in range(n_classes):
                SR.check_row(got[c * 11:(c + 1) * 11], want[c])
            say("both routes agree within the test tolerances (tests/summary_ref.py: check_row), every class")

    say()
    say("## slope_class_plane, one 4096 x 4096 scene, edges 5 / 15 / 30 degrees, cell 10 m")
    y, x = np.mgrid[0:4096, 0:4096].astype(np.float32)
    z = (350 + 120 * np.sin(x / 70.0) * np.cos(y / 50.0) + np.random.RandomState(1).uniform(-1, 1, x.shape)).astype(np.float32)
    scenes = D.DeviceScenes(lr_dem=[z[..., None]], hr_dem=[z[..., None]], relative=True, elev_min=-80, elev_max=933, elev_log=True,
                            device="cuda:0")
    slope = lambda: SM.slope_class_plane(scenes, [5.0, 15.0, 30.0], 10.0)                                               # noqa: E731
    for _ in range(3):
        plane = slope()
    s0 = lib.jspsr_launch_count(b"slope_classes")
    slope()
    assert lib.jspsr_launch_count(b"slope_classes") == s0 + 1
    t = [events(torch, slope, args.iters) for _ in range(args.reps)]
    moved = 5 * 4096 * 4096
    say(f"slope_class_plane (call, one launch): {spread(t, 'us')}")
    say(f"bytes it must move: {moved / 1e6:.1f} MB (4 B read + 1 B written per pixel) -> {moved / statistics.median(t) / 1e3:.0f} GB/s "
        "of whole-call time (allocation of the plane included)")
    say(f"classes: {np.bincount(plane.cpu().numpy(), minlength=4).tolist()}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
