"""K19 (masked losses, csrc/train_step.hip + csrc/loss_terms.hip; the batch's validity plane, csrc/batch.hip) on one MI355X.

(8,1,512,512) pairs with 0 %, 1 % and 50 % of the pixels void; the masked entries against the UNMASKED entries of the same
tree on the same buffers, at the C ABI with preallocated buffers (what the autograd functions of jspsr_amd/losses.py call;
through Python the pair is bound by the host's enqueue time, reported once at the end).  Device events around `iters`
calls, warmed up, the two legs alternating within a repetition; median and spread of the repetitions.

Traffic expectation, bytes per element per pass (every pass streams its tensors once; the eight neighbour taps of the Sobel
stencil and of its adjoint come from cache):
  MultiLoss forward    pred 4 + gt 4 read, sign bytes 2 written                       = 10   masked + 1 (plane)  -> 11 / 10
  MultiLoss backward   pred 4 + gt 4 + sign bytes 2 read, gradient 4 written          = 14   masked + 1          -> 15 / 14
  five keys forward    the above + BerHu's max pass 8 + the sum pass 8                = 26   masked + 3          -> 29 / 26
  five keys backward   the above + pred 4 + gt 4 + gradient 4 read and 4 written      = 30   masked + 2          -> 32 / 30
  (five keys = L1, L2, Grad, Berhu, BCE).  The tensors of this shape are 8 MiB each and stay in the Infinity Cache between
  the calls of a loop, so the ratios measure issue and latency as much as traffic.
  jspsr_batch_valid    1 byte read + 1 written per pixel; jspsr_batch_make with lr_dem, hr_dem, image and a 15-channel mask
                       reads 26 and writes 80: 2 / 106 of its traffic.
Usage: python tools/bench_masked_loss.py [--reps R] [--iters N] [--label TEXT] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (8, 1, 512, 512)
FIVE = {"L1": 1, "L2": 1, "Grad": 0.1, "Berhu": 0.2, "BCE": 0.5}


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
    import numpy as np
    import torch
    from jspsr_amd import _lib, data as D, losses as L
    assert torch.cuda.is_available(), "bench_masked_loss needs the MI355X"
    lib = _lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def legs(name, masked, plain, expect):
        for _ in range(5):
            masked()
            plain()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.reps):
            a.append(events(torch, masked, args.iters))
            b.append(events(torch, plain, args.iters))
        say(f"{name:<22} masked  : {spread(a)}")
        say(f"{name:<22} unmasked: {spread(b)}")
        say(f"{name:<22} masked / unmasked (medians): {statistics.median(a) / statistics.median(b):.3f}; expectation {expect}")

    B, C, H, W = SHAPE
    n = B * C * H * W
    say(f"# K19, masked losses; {torch.cuda.get_device_name(0)}; code: {args.label}")
    say(f"# {SHAPE} pairs; us per call by device events around {args.iters} calls at the C ABI, legs alternating within a repetition")
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(SHAPE, generator=g).cuda()
    pred = (gt + 0.05 * torch.randn(SHAPE, generator=g).cuda()).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    spec = L._Spec(FIVE)
    u8 = lambda nbytes: torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")      # noqa: E731
    ws, wsv = u8(lib.jspsr_loss_workspace_bytes(B * C, H, W)), u8(lib.jspsr_loss_valid_workspace_bytes(B * C, H, W))
    ms, msv = u8(lib.jspsr_loss_menu_workspace_bytes(spec.terms, B * C, H, W)), u8(lib.jspsr_loss_menu_valid_workspace_bytes(spec.terms, B * C, H, W))
    losses, out, gp = torch.empty(4, device="cuda"), torch.empty(len(FIVE) + 1, device="cuda"), torch.empty_like(pred)
    P, G, LS, O, GP = pred.data_ptr(), gt.data_ptr(), losses.data_ptr(), out.data_ptr(), gp.data_ptr()
    w = (1.0, 1.0, 0.1)
    for share in (0.0, 0.01, 0.5):
        plane = (torch.rand(SHAPE, generator=g) >= share).to(torch.uint8).cuda()
        V = plane.data_ptr()
        say()
        say(f"## {share * 100:.0f} % void ({int(plane.sum())} of {n} elements valid)")
        fwd_m = lambda: lib.jspsr_loss_valid_forward(P, G, V, *w, LS, wsv.data_ptr(), B * C, H, W, st)          # noqa: E731
        fwd_p = lambda: lib.jspsr_loss_forward(P, G, *w, LS, ws.data_ptr(), B * C, H, W, st)                     # noqa: E731
        bwd_m = lambda: lib.jspsr_loss_valid_backward(P, G, V, None, *w, GP, wsv.data_ptr(), B * C, H, W, st)    # noqa: E731
        bwd_p = lambda: lib.jspsr_loss_backward(P, G, None, *w, GP, ws.data_ptr(), B * C, H, W, st)              # noqa: E731

        def five_fwd_m():
            lib.jspsr_loss_valid_forward(P, G, V, *spec.base_w, LS, wsv.data_ptr(), B * C, H, W, st)
            lib.jspsr_loss_menu_valid_forward(P, G, V, spec.terms, B * C, H, W, len(FIVE), spec.c_slots, spec.c_weights, LS, O, msv.data_ptr(), st)

        def five_fwd_p():
            lib.jspsr_loss_forward(P, G, *spec.base_w, LS, ws.data_ptr(), B * C, H, W, st)
            lib.jspsr_loss_menu_forward(P, G, spec.terms, B * C, H, W, len(FIVE), spec.c_slots, spec.c_weights, LS, O, ms.data_ptr(), st)

        def five_bwd_m():
            lib.jspsr_loss_valid_backward(P, G, V, None, *spec.base_w, GP, wsv.data_ptr(), B * C, H, W, st)
            lib.jspsr_loss_menu_valid_backward(P, G, V, spec.terms, B * C, H, W, spec.c_slot_w, None, GP, msv.data_ptr(), st)

        def five_bwd_p():
            lib.jspsr_loss_backward(P, G, None, *spec.base_w, GP, ws.data_ptr(), B * C, H, W, st)
            lib.jspsr_loss_menu_backward(P, G, spec.terms, B * C, H, W, spec.c_slot_w, None, GP, ms.data_ptr(), st)

        legs("MultiLoss forward", fwd_m, fwd_p, "11 / 10 = 1.100")
        legs("MultiLoss backward", bwd_m, bwd_p, "15 / 14 = 1.071")
        legs("five keys forward", five_fwd_m, five_fwd_p, "29 / 26 = 1.115")
        legs("five keys backward", five_bwd_m, five_bwd_p, "32 / 30 = 1.067")
        if share == 0.0:
            five_fwd_m(); five_bwd_m()
            a = (losses.clone(), out.clone(), gp.clone())
            five_fwd_p(); five_bwd_p()
            assert all(torch.equal(x, y) for x, y in zip(a, (losses, out, gp)))
            say("all-ones plane: the masked calls have the unmasked calls' bits, every value and every gradient element")
    # through Python (autograd function, allocations): the host's enqueue time bounds the pair
    say()
    plane = (torch.rand(SHAPE, generator=g) >= 0.01).cuda()
    crit = L.get_criterion(FIVE)

    def py(valid):
        x = pred.detach().requires_grad_()
        (crit(x, gt, valid=valid) if valid is not None else crit(x, gt))["Total"].backward()

    legs("five keys, Python pair", lambda: py(plane), lambda: py(None), "61 / 56 = 1.089 if the device were the bound")

    # K9: the plane of a batch beside the batch itself, B = 8, k = 512
    say()
    rs = np.random.RandomState(2)
    side, k, nb = 1024, 512, 8
    hr = [rs.uniform(150, 400, (side, side, 1)).astype(np.float32) for _ in range(2)]
    lr = [h + 1 for h in hr]
    img = [rs.randint(0, 256, (side, side, 3)).astype(np.uint8) for _ in range(2)]
    msk = [(rs.rand(side, side, 15) < 0.1).astype(np.uint8) for _ in range(2)]
    S = D.DeviceScenes(lr, hr, image=img, mask=msk, relative=True, elev_min=-80, elev_max=933, elev_log=True, scale_mask=True,
                       valid=[rs.rand(side, side) < 0.9 for _ in range(2)])
    rows = np.zeros((nb, 8), dtype=np.int32)
    for b in range(nb):
        rows[b, :4] = (b % 2, rs.randint(0, side - k), rs.randint(0, side - k), (b * 5) % 16)
        rows[b, 4] = np.float32(S.base[b % 2]).view(np.int32)
    table = torch.from_numpy(rows).cuda()
    outs = {kind: (torch.empty((nb, S.channels[kind], k, k), device="cuda"), 0) for kind in S.kinds}
    args6 = D.ctypes_arrays(S, outs)
    vout = torch.empty((nb, 1, k, k), dtype=torch.uint8, device="cuda")
    pl = S.store["valid"]
    make = lambda: lib.jspsr_batch_make(*args6, S.scene_table.data_ptr(), len(S), table.data_ptr(), nb, k, S.flags,          # noqa: E731
                                        float(S.elev_min), float(S.elev_max), len(S.mask_channel) + 1, st)
    valid = lambda: lib.jspsr_batch_valid(pl.data_ptr(), pl.numel(), vout.data_ptr(), S.scene_table.data_ptr(), len(S),     # noqa: E731
                                          table.data_ptr(), nb, k, st)
    assert make() == 0 and valid() == 0
    for _ in range(5):
        make()
        valid()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(args.reps):
        a.append(events(torch, valid, args.iters))
        b.append(events(torch, make, args.iters))
    say(f"## the batch's plane, B = {nb}, k = {k}, codes mixed (lr_dem, hr_dem, image, 15-channel mask in the batch)")
    say(f"jspsr_batch_valid: {spread(a)}")
    say(f"jspsr_batch_make : {spread(b)}")
    say(f"valid / make (medians): {statistics.median(a) / statistics.median(b):.3f}; expectation by traffic 2 / 106 = {2 / 106:.3f} "
        "(a 2 MiB output: the launch, not the traffic, bounds the plane's kernel)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
