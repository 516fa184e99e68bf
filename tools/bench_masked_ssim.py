"""K23 (SSIM over a validity plane, the "window" rule; csrc/loss_terms.hip) on one MI355X.

(8,1,512,512) pairs with 0 %, 0.1 % and 1 % of the pixels void; the masked entries against the UNMASKED entries of the same
tree on the same buffers, at the C ABI with preallocated buffers (what the autograd functions of jspsr_amd/losses.py and
metrics.ssim_tiles call).  Device events around `iters` calls, warmed up, the two legs alternating within a repetition; median
and spread of the repetitions.

Expectation, SSIM forward: per map element the unmasked kernel reads about 8 bytes (pred and gt, the 10-pixel halo of a
32 x 32 tile staged again by its neighbours) and writes 12 (alpha, beta, gamma); the plane adds 1 byte per staged pixel, so
by traffic the ratio would be near 21 / 20, and with the extra byte reads of the separable void count in LDS (one byte tap
beside every two float taps of the horizontal pass) a ratio near 1.1 is expected.  The backward reads the plane once per
pixel beside pred, gt and the gradient (1 byte on about 28): near 1.04.  The tensors of this shape are 8 MiB each and stay
in the Infinity Cache between the calls of a loop, so the ratios measure issue and LDS work as much as traffic.
ssim_tiles against today's meter (B `metrics.ssim` calls on prepared samples, two launches each and a crop copy): the same
arithmetic in 2 launches instead of 2 B, so the gain is the launches' at 128 x 128 and shrinks towards 1 at 512 x 512.
Usage: python tools/bench_masked_ssim.py [--reps R] [--iters N] [--label TEXT] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (8, 1, 512, 512)
FIVE = {"L1": 1, "L2": 1, "Grad": 0.1, "SSIM": 0.5, "Berhu": 0.2}


def spread(xs, unit="us"):
    return f"median {statistics.median(xs):9.2f}  min {min(xs):9.2f}  max {max(xs):9.2f} {unit} (n={len(xs)}: " + \
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--label", default="working tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from jspsr_amd import _lib, losses as L, metrics as M
    assert torch.cuda.is_available(), "bench_masked_ssim needs the MI355X"
    lib = _lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def legs(name, new, old, expect, names=("masked  ", "unmasked")):
        for _ in range(5):
            new()
            old()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.reps):
            a.append(events(torch, new, args.iters))
            b.append(events(torch, old, args.iters))
        say(f"{name:<24} {names[0]}: {spread(a)}")
        say(f"{name:<24} {names[1]}: {spread(b)}")
        say(f"{name:<24} {names[0].strip()} / {names[1].strip()} (medians): {statistics.median(a) / statistics.median(b):.3f}; expectation {expect}")

    B, C, H, W = SHAPE
    say(f"# K23, SSIM over a validity plane (window rule); {torch.cuda.get_device_name(0)}; code: {args.label}")
    say(f"# {SHAPE} pairs; us per call by device events around {args.iters} calls at the C ABI, legs alternating within a repetition")
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(SHAPE, generator=g).cuda()
    pred = (gt + 0.05 * torch.randn(SHAPE, generator=g).cuda()).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    spec, only = L._Spec(FIVE, "window"), L._Spec({"SSIM": 1.0}, "window")
    u8 = lambda nbytes: torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")      # noqa: E731
    ws, wsv = u8(lib.jspsr_loss_workspace_bytes(B * C, H, W)), u8(lib.jspsr_loss_valid_workspace_bytes(B * C, H, W))
    work = {}
    for key, s in (("five", spec), ("ssim", only)):
        work[key] = (u8(lib.jspsr_loss_menu_valid_ssim_workspace_bytes(s.terms, B * C, H, W, 1)),
                     u8(lib.jspsr_loss_menu_workspace_bytes(s.terms, B * C, H, W)))
    losses, gp = torch.empty(4, device="cuda"), torch.empty_like(pred)
    out = torch.empty(len(FIVE) + 1, device="cuda")
    P, G, LS, O, GP = pred.data_ptr(), gt.data_ptr(), losses.data_ptr(), out.data_ptr(), gp.data_ptr()
    for share in (0.0, 0.001, 0.01):
        plane = (torch.rand(SHAPE, generator=g) >= share).to(torch.uint8).cuda()
        V = plane.data_ptr()
        _, cnt = M.ssim_tiles(pred, gt, "piq", 0.0, valid=plane)
        say()
        say(f"## {share * 100:.1f} % void ({int(plane.sum())} of {plane.numel()} pixels valid, {int(cnt.sum())} of {B * C * (H - 10) * (W - 10)} "
            "map elements counted)")

        def fwd_m(s, key, base):
            if base:
                lib.jspsr_loss_valid_forward(P, G, V, *s.base_w, LS, wsv.data_ptr(), B * C, H, W, st)
            lib.jspsr_loss_menu_valid_ssim_forward(P, G, V, s.terms, B * C, H, W, 1, len(s.keys), s.c_slots, s.c_weights,
                                                   LS if base else None, O, work[key][0].data_ptr(), st)

        def fwd_p(s, key, base):
            if base:
                lib.jspsr_loss_forward(P, G, *s.base_w, LS, ws.data_ptr(), B * C, H, W, st)
            lib.jspsr_loss_menu_forward(P, G, s.terms, B * C, H, W, len(s.keys), s.c_slots, s.c_weights, LS if base else None, O,
                                        work[key][1].data_ptr(), st)

        def bwd_m(s, key, base):
            if base:
                lib.jspsr_loss_valid_backward(P, G, V, None, *s.base_w, GP, wsv.data_ptr(), B * C, H, W, st)
            lib.jspsr_loss_menu_valid_ssim_backward(P, G, V, s.terms, B * C, H, W, 1, s.c_slot_w, None, GP, work[key][0].data_ptr(), st)

        def bwd_p(s, key, base):
            if base:
                lib.jspsr_loss_backward(P, G, None, *s.base_w, GP, ws.data_ptr(), B * C, H, W, st)
            lib.jspsr_loss_menu_backward(P, G, s.terms, B * C, H, W, s.c_slot_w, None, GP, work[key][1].data_ptr(), st)

        legs("SSIM alone forward", lambda: fwd_m(only, "ssim", False), lambda: fwd_p(only, "ssim", False), "near 1.1")
        legs("SSIM alone backward", lambda: bwd_m(only, "ssim", False), lambda: bwd_p(only, "ssim", False), "near 1.04")
        legs("five keys forward", lambda: fwd_m(spec, "five", True), lambda: fwd_p(spec, "five", True),
             "K19's 1.1 on the pointwise passes, 1.1 on SSIM: near 1.1")
        legs("five keys backward", lambda: bwd_m(spec, "five", True), lambda: bwd_p(spec, "five", True), "near 1.05")
        if share == 0.0:
            fwd_m(spec, "five", True); bwd_m(spec, "five", True)
            a = (losses.clone(), out.clone(), gp.clone())
            fwd_p(spec, "five", True); bwd_p(spec, "five", True)
            assert all(torch.equal(x, y) for x, y in zip(a, (losses, out, gp)))
            say("all-ones plane: the masked calls have the unmasked calls' bits, every value and every gradient element")

    # the meters: all tiles from one call against one metrics.ssim call per prepared sample (today's unmasked meter)
    for side in (128, 512):
        p, q = pred[:, :, :side, :side].contiguous(), gt[:, :, :side, :side].contiguous()
        plane = (torch.rand((B, 1, side, side), generator=g) >= 0.001).to(torch.uint8).cuda()
        say()
        say(f"## ssim_tiles, B = {B} tiles of {side} x {side}, border 0.05, 0.1 % void")
        for package in ("piq", "local"):
            win = (ctypes.c_float * 11)(*M.local_window().tolist()) if package == "local" else None
            same = int(package == "local")
            wt = u8(max(lib.jspsr_ssim_tiles_workspace_bytes(B, side, side, 0.05, same), 16))
            vals, cnts = torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")

            def tiles(v):
                lib.jspsr_ssim_tiles_forward(p.data_ptr(), q.data_ptr(), v, B, side, side, 0.05, same, win, vals.data_ptr(),
                                             cnts.data_ptr(), wt.data_ptr(), st)

            def per_sample():
                pp, gg = M.prepare(p, q, 0.05)
                return [M.ssim(pp[i:i + 1], gg[i:i + 1], package) for i in range(B)]

            legs(f"{package} ssim_tiles, plane", lambda: tiles(plane.data_ptr()), lambda: tiles(None), "near 1.1", ("masked  ", "unmasked"))
            legs(f"{package} tiles vs per-sample", lambda: M.ssim_tiles(p, q, package, 0.05, valid=plane), per_sample,
                 "2 launches against 2 B and B crop copies: well below 1 at 128, towards 1 at 512", ("ssim_tiles(valid)", "B x metrics.ssim  "))
            tiles(None)
            assert torch.equal(vals, torch.stack(per_sample()))
        say("without a plane every tile has the bits of metrics.ssim on the prepared sample alone")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
