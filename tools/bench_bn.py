"""K4 micro-benchmark: the BatchNorm backward (reduce + finalize + apply; 5 tensor passes: dy, x read twice, dx written) and
forward apply as the models call them, effective GB/s over the bytes they must move.

--mode1: the BatchNorm + residual + ReLU backward alone (relu mode 1 with the residual gradient wanted: reduce + finalize +
apply), by arm -- the saved output y as the mask (7 tensor passes: the reduce pass writes the masked gradient, the apply
pass reads it back; 8 passes in a tree from before that) and the forward's bit mask (6 + 1/16 passes) -- with the bytes per
call from the shapes, GB/s and the share of the 8 TB/s HBM peak.  Run the same file in an older tree for its arm: the arms
a tree does not have are left out.

--shortcut: the two BatchNorm backwards of a projecting residual block, whole call, by the same rule (300 warm-up calls, the
median of 5 windows): bn2's call with the bit mask and then the shortcut BatchNorm's on the masked gradient (11.06 passes)
against the pair call (8.12 passes), on 8 x 512^2 x 64 and 8 x 256^2 x 128 in bf16."""
import inspect
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jspsr_amd import kernels as K  # noqa: E402

SHAPES = [(8, 512, 512, 64), (8, 256, 256, 128), (8, 128, 128, 256), (8, 64, 64, 512), (8, 512, 512, 32)]


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def steady(fn, reps=5, warm=300, n=40):
    """Median and (min, max) over `reps` windows of `n` back-to-back calls, each window straight behind `warm` warm-up calls."""
    ts = []
    for _ in range(reps):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n * 1e-3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def mode1():
    has_mask = "mask" in inspect.signature(K.bn_backward).parameters
    passes_y = float(os.environ.get("BENCH_BN_PASSES_Y", "7" if has_mask else "8"))      # an older tree: 8 passes
    for B, H, W, C in [(8, 512, 512, 64), (8, 256, 256, 128)]:
        mk = lambda: torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
        x, res, dy = mk(), mk(), mk()
        gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
        T = x.numel() * x.element_size()
        kw = dict(want_mask=True) if has_mask else {}
        y, mean, invstd, *mask = K.bn_forward(x, gamma, beta, None, None, 0.1, 1e-5, True, True, res, 1.0, **kw)
        arms = [(f"mask from y, {passes_y:g} passes", passes_y,
                 lambda: K.bn_backward(dy, y, x, gamma, mean, invstd, True, 1, 1.0, want_dres=True))]
        if has_mask:
            arms.append(("bit mask, 6.06 passes", 6.0625,
                         lambda: K.bn_backward(dy, None, x, gamma, mean, invstd, True, 1, 1.0, want_dres=True, mask=mask[0])))
        for name, passes, fn in arms:
            med, lo, hi = steady(fn)
            gbs = passes * T / med / 1e9
            print(f"bf16 B{B} {H}x{W}x{C} bn_backward mode 1 + dres [{name}]: median {med*1e6:7.1f} us (min {lo*1e6:.1f}, max {hi*1e6:.1f}) "
                  f"{passes * T / 1e6:7.1f} MB {gbs:6.0f} GB/s = {gbs / 80:4.1f} % of 8 TB/s", flush=True)


def shortcut():
    """A projection block's two BatchNorm backwards: bn2 (bit mask, masked gradient out) then the shortcut's on that gradient
    (11.06 passes, 6 launches) against the pair call (8.12 passes, 3 launches); a tree without the pair call times its arm."""
    for B, H, W, C in [(8, 512, 512, 64), (8, 256, 256, 128)]:
        mk = lambda: torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
        z2, zd, dy = mk(), mk(), mk()
        g2, b2, gd, bd = (torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1,
                          torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1)
        T = z2.numel() * z2.element_size()
        affd, md, idd = K.bn_forward(zd, gd, bd, None, None, 0.1, 1e-5, True, False, stats_only=True)
        y, m2, i2, mask = K.bn_forward(z2, g2, b2, None, None, 0.1, 1e-5, True, True, zd, 1.0, res_affine=affd, want_mask=True)

        def two_calls():
            _, dres, _, _ = K.bn_backward(dy, None, z2, g2, m2, i2, True, 1, 1.0, want_dres=True, mask=mask)
            K.bn_backward(dres, None, zd, gd, md, idd, True, 0, 1.0)

        arms = [("two calls, 11.06 passes", 11.0625, two_calls)]
        if hasattr(K, "bn_backward_pair"):
            arms.append(("pair call, 8.12 passes", 8.125, lambda: K.bn_backward_pair(dy, mask, z2, g2, m2, i2, True, 1.0, zd, gd, md, idd, True)))
        for name, passes, fn in arms:
            med, lo, hi = steady(fn)
            gbs = passes * T / med / 1e9
            print(f"bf16 B{B} {H}x{W}x{C} bn2 + shortcut bn backward [{name}]: median {med*1e6:7.1f} us (min {lo*1e6:.1f}, max {hi*1e6:.1f}) "
                  f"{passes * T / 1e6:7.1f} MB {gbs:6.0f} GB/s = {gbs / 80:4.1f} % of 8 TB/s", flush=True)


if "--mode1" in sys.argv:
    mode1()
    sys.exit(0)
if "--shortcut" in sys.argv:
    shortcut()
    sys.exit(0)

for dtype in (torch.bfloat16,):
    for B, H, W, C in SHAPES:
        x = torch.randn(B, H, W, C, device="cuda").to(dtype)
        dy = torch.randn(B, H, W, C, device="cuda").to(dtype)
        gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        y, mean, invstd = K.bn_forward(x, gamma, beta, rm, rv, 0.1, 1e-5, True, relu=True)
        nbytes = x.numel() * x.element_size()
        t_f = timeit(lambda: K.bn_forward(x, gamma, beta, rm, rv, 0.1, 1e-5, True, relu=True))
        t_b = timeit(lambda: K.bn_backward(dy, None, x, gamma, mean, invstd, True, 2, beta=beta))
        t_by = timeit(lambda: K.bn_backward(dy, y, x, gamma, mean, invstd, True, 1))
        print(f"{str(dtype)[6:]} B{B} {H}x{W}x{C}: forward (stats + apply, 3 passes) {t_f*1e6:7.1f} us {3*nbytes/t_f/1e9:6.0f} GB/s | "
              f"backward, mask from x (5 passes) {t_b*1e6:7.1f} us {5*nbytes/t_b/1e9:6.0f} GB/s | mask from y (6 passes) {t_by*1e6:7.1f} us {6*nbytes/t_by/1e9:6.0f} GB/s", flush=True)
