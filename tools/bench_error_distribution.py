"""K21 (the whole-set error distribution, jspsr_amd/summary.py: pooled_histogram / kde_curves) on one MI355X.

Two sizes -- one 4096 x 4096 pair (1 candidate) and 8 candidates of 2048 x 2048 -- and three error shapes:
  spread   errors of sigma = 1.3 m: a good model's, thousands of occupied bins
  hot      the same with half of the errors exactly 0 (a baseline that equals the ground truth over water): the bin of +0
  masked   the spread errors under a plane that masks 50 %
  histogram pass   `pooled_histogram` (jspsr_errdist_hist_forward), device events around `iters` calls, warmed up; the
                   effective bytes/s against the (n_cand + 1) x 4 B per element the pass has to read (+ 1 B with a plane), and
                   the hot-bin slowdown over the spread case.  No ratio is fixed in advance: nobody has measured integer LDS
                   adds at this contention on this part.  --rounds 0 / 1 / 2 selects how many ballot-aggregated rounds the LDS
                   add takes before the plain adds (JSPSR_ERRDIST_ROUNDS, read once when the library loads).
  curve pass       `kde_curves` (jspsr_errdist_kde_forward) on that histogram.
  yardsticks       `pooled_rows` on the same buffers (K12 reads the same bytes, 16 launches); and the route the calls
                   replace: a device-to-host copy of the rasters, numpy filter, astype(float16), np.unique, and the curve from
                   those counts in numpy (host clock to the result; skipped with --no-host).  The two routes' histograms must
                   be equal and the curves agree within the test tolerances (asserted).
Usage: python tools/bench_error_distribution.py [--reps R] [--iters N] [--rounds K] [--no-host] [--label TEXT] [--out FILE] [--append]"""
import argparse
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
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--label", default="working tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.rounds is not None:
        os.environ["JSPSR_ERRDIST_ROUNDS"] = str(args.rounds)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from jspsr_amd import _lib, summary as SM
    from tests import errdist_ref as ER
    assert torch.cuda.is_available(), "bench_error_distribution needs the MI355X"
    _lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# K21, error distribution; {torch.cuda.get_device_name(0)}; code: {args.label}; "
        f"aggregated rounds of the LDS add: {os.environ.get('JSPSR_ERRDIST_ROUNDS', '2 (default)')}")
    say(f"# us per call by device events around {args.iters} calls, {args.reps} repetitions")
    g = torch.Generator().manual_seed(1)
    for side, n_cand in ((4096, 1), (2048, 8)):
        n = side * side
        gt = (torch.rand(n, generator=g) * 500 + 100).cuda()
        noise = [1.3 * torch.randn(n, generator=g).cuda() * (1 + 0.2 * c) for c in range(n_cand)]
        zero = [(torch.rand(n, generator=g) < 0.5).cuda() for _ in range(n_cand)]
        plane = (torch.rand(n, generator=g) >= 0.5).to(torch.uint8).cuda()
        wins = [(0, side, side, (0, side), [(0, side)] * n_cand)]
        shapes = {"spread": ([gt + e for e in noise], None),
                  "hot": ([torch.where(z, gt, gt + e) for z, e in zip(zero, noise)], None),
                  "masked": ([gt + e for e in noise], plane)}
        say()
        say(f"## {n_cand} candidate(s) of {side} x {side}")
        med = {}
        for name, (cands, valid) in shapes.items():
            hist_call = lambda: SM.pooled_histogram(cands, gt, wins, valid=valid)                            # noqa: E731
            hist, counts, key0 = hist_call()
            kde_call = lambda: SM.kde_curves(hist, key0)                                                    # noqa: E731
            rows_call = lambda: SM.pooled_rows(cands, gt, wins, 1, VMAX, valid=valid)                       # noqa: E731
            for _ in range(3):
                hist_call()
                kde_call()
                rows_call()
            torch.cuda.synchronize()
            a, b, c = [], [], []
            for _ in range(args.reps):
                a.append(events(torch, hist_call, args.iters))
                b.append(events(torch, kde_call, args.iters))
                c.append(events(torch, rows_call, max(1, args.iters // 5)))
            med[name] = statistics.median(a)
            nbytes = n * ((n_cand + 1) * 4 + (1 if valid is not None else 0))
            occupied = [int(v) for v in (hist > 0).sum(dim=1).cpu()]
            top = [float(v) for v in (hist.max(dim=1).values.double() / counts[:, 1].clamp(min=1).double()).cpu()]
            say(f"### {name}: occupied bins per candidate {occupied}, share of the fullest bin {[round(t, 3) for t in top]}")
            say(f"histogram pass pooled_histogram: {spread(a, 'us')}")
            say(f"  effective {nbytes / med[name] / 1e6:.3f} TB/s of the {nbytes / 1e6:.1f} MB the pass has to read "
                f"({(n_cand + 1) * 4 + (1 if valid is not None else 0)} B per element)")
            say(f"curve pass kde_curves (200 points)  : {spread(b, 'us')}")
            say(f"yardstick pooled_rows (K12{'/K18' if valid is not None else ''}, 16 launches): {spread(c, 'us')}")
            if args.no_host:
                continue

            def host_leg():
                t = gt.cpu().numpy()
                keep = None if valid is None else valid.cpu().numpy() != 0
                out = []
                for cand in cands:
                    e = cand.cpu().numpy() - t                                                              # the copies
                    e = e if keep is None else e[keep]
                    x = e[(e >= -5) & (e <= 5)].astype("float16")
                    u, cnt = np.unique(x.view(np.uint16), return_counts=True)
                    v, w = u.view(np.float16).astype(np.float64), cnt.astype(np.float64)
                    m = w.sum()
                    mean = (w * v).sum() / m
                    bw = np.sqrt((w * (v - mean) ** 2).sum() / (m - 1)) * m ** -0.2
                    sup = np.linspace(v.min() - 0.5 * bw, v.max() + 0.5 * bw, 200)
                    den = np.array([(w * np.exp(-(s - v) ** 2 / (2 * bw * bw))).sum() for s in sup]) / (m * bw * np.sqrt(2 * np.pi))
                    out.append((u, cnt, sup, den))
                return out

            def dev_leg():
                h, k, k0 = SM.pooled_histogram(cands, gt, wins, valid=valid)
                s, d, st = SM.kde_curves(h, k0)
                return torch.cat((s.reshape(-1), d.reshape(-1), st.reshape(-1), k.double().reshape(-1))).cpu().numpy(), h   # one copy back

            dev_leg()
            ta = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got, h = dev_leg()
                ta.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            want = host_leg()
            tb = (time.perf_counter() - t0) * 1e3
            say(f"both passes + one copy back, host clock to the curves: {spread(ta, 'ms')}")
            say(f"the route replaced (copies, filter, astype(float16), np.unique, numpy curve), {os.environ.get('OMP_NUM_THREADS', '?')} OMP: "
                f"{tb:.1f} ms (1 run); host / device {tb / statistics.median(ta):.0f}")
            h = h.cpu().numpy()
            for ci, (u, cnt, sup, den) in enumerate(want):
                ref = np.zeros(h.shape[1], dtype=np.int64)
                ref[ER.f16_key(u) - key0] = cnt
                assert np.array_equal(h[ci], ref), (name, ci)
                ER.check_curve(got[ci * 200:(ci + 1) * 200], got[(n_cand + ci) * 200:(n_cand + ci + 1) * 200], sup, den, f"{name} {ci}")
            say("both routes agree: histograms equal, curves within the test tolerances")
        say(f"hot-bin slowdown over the spread case (medians): {med['hot'] / med['spread']:.2f}; masked / spread: {med['masked'] / med['spread']:.2f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
