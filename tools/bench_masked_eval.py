"""K20 (per-tile scores over valid pixels, jspsr_amd/metrics.py: batch_scores(valid=...)) on one MI355X.

B = 8 tiles of 128 x 128 (the LDS path, one launch) and of 512 x 512 (the streaming path, 27 launches), border 0, log scaling,
with 0 %, 1 % and 50 % of the pixels masked:
  masked vs unmasked   `batch_scores(valid=plane)` (jspsr_scores_batch_valid_forward) against `batch_scores` (K10's
                       jspsr_scores_batch_forward) on the same buffers.  Device events around `iters` calls, warmed up, the two
                       legs alternating within a repetition; median and spread of the repetitions.  The expectation to confirm
                       or refute: the mask travels inside the de-scaled prediction, so the masked call reads one byte per pixel
                       more in the first pass (9 B against 8 B there) and nothing more in the Sobel pass and the twelve select
                       passes: close to the unmasked call, and below it at 50 %, where half the histogram increments vanish.
  masked vs host       the route the call replaces: a device-to-host copy of both batches and the plane, boolean indexing per
                       tile, np.sort and the fp64 RMSE.  Host clock to the result, both legs; N must be equal (asserted), the
                       agreement of the values is reported (numpy's expf need not be the device's to the last bit).
Usage: python tools/bench_masked_eval.py [--reps R] [--iters N] [--host-reps H] [--label TEXT] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMIN, VMAX = -80.0, 929.0
B = 8


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
    from jspsr_amd import _lib, metrics as M
    assert torch.cuda.is_available(), "bench_masked_eval needs the MI355X"
    lib = _lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def ulps(a, b):
        a, b = np.float32(a), np.float32(b)
        return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b), np.float32(1e-30))))

    say(f"# K20, per-tile scores over valid pixels; {torch.cuda.get_device_name(0)}; code: {args.label}")
    say(f"# B = {B} tiles, border 0, log scaling; us per call by device events around {args.iters} calls, legs alternating within a "
        "repetition")
    g = torch.Generator().manual_seed(1)
    for side, label, per_call in ((128, b"scores_batch_valid (lds)", 1), (512, b"scores_batch_valid (stream)", 27)):
        n = side * side
        gt = (torch.rand(B, 1, side, side, generator=g) * 0.5 + 0.3).cuda()
        pred = (gt + 0.002 * torch.randn(B, 1, side, side, generator=g).cuda()).clamp(0, 1)
        for share in (0.0, 0.01, 0.5):
            say()
            plane = (torch.rand(B, 1, side, side, generator=g) >= share).to(torch.uint8).cuda()
            gt_m = torch.where(plane != 0, gt, torch.full_like(gt, -32767.0))                    # a ground truth with voids
            masked = lambda: M.batch_scores(pred, gt_m, VMIN, VMAX, 0.0, True, valid=plane)      # noqa: E731
            plain = lambda: M.batch_scores(pred, gt_m, VMIN, VMAX, 0.0, True)                    # noqa: E731
            for _ in range(3):
                masked()
                plain()
            torch.cuda.synchronize()
            v0 = lib.jspsr_launch_count(label)
            rows, counts = masked()
            assert lib.jspsr_launch_count(label) == v0 + per_call
            a, b = [], []
            for _ in range(args.reps):
                a.append(events(torch, masked, args.iters))
                b.append(events(torch, plain, args.iters))
            ma, mb = statistics.median(a), statistics.median(b)
            say(f"## {side} x {side} ({label.decode()}, {per_call} launch{'es' if per_call > 1 else ''}), {share * 100:.0f} % masked "
                f"({int(counts[:, 0].sum())} of {B * n} pixels scored)")
            say(f"masked   batch_scores(valid=): {spread(a, 'us')}")
            say(f"unmasked batch_scores        : {spread(b, 'us')}")
            say(f"masked / unmasked (medians): {ma / mb:.3f}; expectation: close to 1 (first pass 9 B against 8 B per pixel, nothing "
                "more after it), below 1 at 50 %")

            def host_leg():
                p, t, v = pred.cpu().numpy(), gt_m.cpu().numpy(), plane.cpu().numpy()             # the copies
                lg = np.float32(math.log(VMAX - VMIN))
                out = []
                for i in range(B):
                    keep = v[i, 0] != 0
                    e = ((np.exp(p[i, 0] * lg) + np.float32(VMIN)) - (np.exp(t[i, 0] * lg) + np.float32(VMIN)))[keep]
                    s = np.sort(e)
                    med = s[(e.size - 1) // 2]
                    dev = np.sort(np.abs(e - med))
                    le = np.sort(np.abs(e))[round(0.95 * (e.size - 1))]
                    out.append((math.sqrt(np.mean(e.astype(np.float64) ** 2)), med, np.float32(1.4826) * dev[(e.size - 1) // 2], le, e.size))
                return out

            def dev_leg():
                r, c = M.batch_scores(pred, gt_m, VMIN, VMAX, 0.0, True, valid=plane)
                return torch.cat((r.reshape(-1), c.reshape(-1).view(torch.float32))).cpu().numpy()   # one copy back, the counts' bits

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
            grow, gcnt = got[:B * 8].reshape(B, 8), got[B * 8:].view(np.int32).reshape(B, 3)
            worst, med_equal = 0.0, 0
            for i in range(B):
                assert int(gcnt[i, 0]) == want[i][4] == int(counts[i, 0])
                med_equal += int(grow[i, 3] == want[i][1])
                worst = max(worst, ulps(grow[i, 2], want[i][0]), ulps(grow[i, 4], want[i][2]), ulps(grow[i, 5], want[i][3]))
            # numpy's expf and the device's may differ in the last bit of an elevation, so the host route is held to the
            # device's by value, not by bits
            say(f"both routes: N equal on all {B} tiles; Median bit-equal on {med_equal} of {B}; RMSE / NMAD / LE95 differ by at most "
                f"{worst:.2f} fp32 ulp")
            say(f"row 0 {M.SCORE_COLUMNS}: {[float(x) for x in rows[0].cpu().numpy()]}")
            if share == 0.0:
                assert rows.cpu().numpy().tobytes() == M.batch_scores(pred, gt, VMIN, VMAX, 0.0, True).cpu().numpy().tobytes()
                say("all-ones plane: the masked call has the unmasked call's bits, all 8 columns")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
