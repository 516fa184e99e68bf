"""K18 (pooled scores over valid pixels, jspsr_amd/summary.py: scores_pooled(valid=...)) on one MI355X.

One 4096 x 4096 raster pair, one candidate, one segment, with 0 %, 1 % and 50 % of the pixels masked:
  masked vs unmasked   `scores_pooled(valid=plane)` (jspsr_summary_valid_forward) against `scores_pooled` (K12's
                       jspsr_summary_forward) on the same buffers.  Device events around `iters` calls, warmed up, the two legs
                       alternating within a repetition; median and spread of the repetitions.  The expectation to confirm or
                       refute: the masked call costs the unmasked one plus one byte per element of traffic per pass -- 1 read
                       of the plane and 1 write of the validity bytes in the first pass, 1 read in each of the 7 select
                       passes, against K12's 4 * (3 + 7) bytes per element: + 22.5 %.
  masked vs host       the route the call replaces: a device-to-host copy of both rasters and the plane, boolean indexing,
                       np.median / NMAD / np.percentile (np.sort underneath) and the fp64 RMSE.  Host clock to the result, both
                       legs; the rows must agree within the test tolerances (asserted).
Usage: python tools/bench_summary_valid.py [--reps R] [--iters N] [--host-reps H] [--label TEXT] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMAX = 933.0


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
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--label", default="working tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import _lib, summary as SM
    from tests import summary_ref as SR
    assert torch.cuda.is_available(), "bench_summary_valid needs the MI355X"
    lib = _lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# K18, pooled scores over valid pixels; {torch.cuda.get_device_name(0)}; code: {args.label}")
    say(f"# one 4096 x 4096 pair, 1 candidate, 1 segment; us per call by device events around {args.iters} calls, legs alternating "
        "within a repetition")
    g = torch.Generator().manual_seed(1)
    n = 4096 * 4096
    gt = (torch.rand(1, 4096, 4096, generator=g) * 500 + 100).cuda()
    pred = gt + 4.0 * torch.randn(1, 4096, 4096, generator=g).cuda()
    for share in (0.0, 0.01, 0.5):
        say()
        plane = (torch.rand(1, 4096, 4096, generator=g) >= share).to(torch.uint8).cuda()
        pred_m = torch.where(plane != 0, pred, torch.full_like(pred, -32767.0))                               # a mask_voids result
        masked = lambda: SM.scores_pooled(pred_m, gt, value_max=VMAX, valid=plane)                            # noqa: E731
        plain = lambda: SM.scores_pooled(pred_m, gt, value_max=VMAX)                                          # noqa: E731
        for _ in range(3):
            masked()
            plain()
        torch.cuda.synchronize()
        v0 = lib.jspsr_launch_count(b"summary_valid_prepare") + lib.jspsr_launch_count(b"summary_valid_select")
        rows, counts = masked()
        assert lib.jspsr_launch_count(b"summary_valid_prepare") + lib.jspsr_launch_count(b"summary_valid_select") == v0 + 16
        a, b = [], []
        for _ in range(args.reps):
            a.append(events(torch, masked, args.iters))
            b.append(events(torch, plain, args.iters))
        ma, mb = statistics.median(a), statistics.median(b)
        say(f"## {share * 100:.0f} % masked ({int(counts[0])} of {n} pixels scored)")
        say(f"masked   scores_pooled(valid=): {spread(a, 'us')}")
        say(f"unmasked scores_pooled        : {spread(b, 'us')}")
        say(f"masked / unmasked (medians): {ma / mb:.3f}; expectation 'unmasked + 1 B per element per pass': "
            f"(40 + 9) / 40 = {49 / 40:.3f}")

        def host_leg():
            p, t, v = pred_m.cpu().numpy().reshape(-1), gt.cpu().numpy().reshape(-1), plane.cpu().numpy().reshape(-1)   # the copies
            e = (p - t)[v != 0]
            med = np.median(e)
            return {"RMSE": math.sqrt(np.mean(e.astype(np.float64) ** 2)), "Median": med,
                    "NMAD": 1.4826 * float(np.median(np.abs(e - med))), "LE95": float(np.percentile(np.abs(e).astype(np.float64), 95)),
                    "N": e.size}

        def dev_leg():
            r, c = SM.scores_pooled(pred_m, gt, value_max=VMAX, valid=plane)
            both = torch.cat((r.double().reshape(-1), c.double())).cpu().numpy()                              # one copy back
            return both

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
        say(f"device call + one copy back, host clock to the result : {spread(ta, 'ms')}")
        say(f"copy to host + boolean indexing + numpy, {torch.get_num_threads()} torch threads / "
            f"{os.environ.get('OMP_NUM_THREADS', '?')} OMP: {spread(tb, 'ms')}")
        say(f"host / device (medians): {statistics.median(tb) / statistics.median(ta):.1f}")
        assert int(got[11]) == want["N"] == int(counts[0])
        assert np.float32(got[1]) == want["Median"]
        worst = max(float(SR.ulps(np.float32(got[j]), want[k])) for j, k in ((0, "RMSE"), (2, "NMAD"), (3, "LE95")))
        assert worst <= 2.0, worst
        say(f"both routes agree: N equal, Median bit-equal, RMSE / NMAD / LE95 within {worst:.2f} fp32 ulp")
        say(f"row (RMSE, Median, NMAD, LE95, PSNR): {[float(x) for x in rows[0, 0, :5].cpu().numpy()]}")
        if share == 0.0:
            assert rows.cpu().numpy().tobytes() == plain().cpu().numpy().tobytes()
            say("all-ones plane: the masked call has the unmasked call's bits, all 11 columns")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
