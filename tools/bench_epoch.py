"""K11's step kernels on their own, and one training epoch timed three ways on the same commit.

1. Kernel bandwidth at the benched model's 43.87 M parameters (fp32 flat buffers): the existing `jspsr_adamw_step` (the
   baseline: the parent commit's kernel, same process, same box, same run) against `jspsr_optim_step` for AdamW, SGD with
   momentum (20 B / parameter), Adam (28) and RMSprop with momentum (28), each without and with the fused gradient range.
   Device events around `--iters` launches after a warm-up; the legs alternate within a repetition; medians of `--reps`.
2. Epoch wall time: `--steps` steps of JSPSR (image + mask, num_feature 32), 8 x 512 x 512, bf16 storage, FlatAdamW,
   L1 + L2 + 0.1 Grad.
     A   `train.train_one_epoch` (one host synchronisation per epoch), without and with monitor_value="grad";
     B   a loop over the same calls with the reference's four `.item()` per step (train/train_utils.py:225-226);
     C   B plus the per-parameter gradient range written with torch operators as get_gradient_range writes it (:127-143).
   Host clock around an epoch that ends in a device synchronise; the legs alternate; medians of `--reps`.
Usage: python tools/bench_epoch.py [--reps R] [--iters I] [--steps S] [--nf F] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jspsr_amd import _lib  # noqa: E402
from jspsr_amd import losses as L  # noqa: E402
from jspsr_amd import optim as O  # noqa: E402
from jspsr_amd import train as TR  # noqa: E402
from jspsr_amd.ddp import GradReducer  # noqa: E402
from oracle import jspsr_ref as R  # noqa: E402

IC = {"lr_dem": 1, "image": 3, "mask": 15}
N_PARAMS = 43_870_000


def line(xs, unit):
    med = statistics.median(xs)
    return med, f"median {med:10.2f} {unit}  min {min(xs):10.2f}  max {max(xs):10.2f}  spread {(max(xs) - min(xs)) / med:6.3f}"


def kernel_bandwidth(reps, iters, out):
    lib = _lib.load()
    dev = "cuda:0"
    p, g, s1, s2 = (torch.randn(N_PARAMS, device=dev) * 0.01 for _ in range(4))
    s1.abs_(), s2.abs_()
    rng = torch.tensor([999.0, -999.0, 0.0, 0.0], device=dev)
    ws = torch.empty(lib.jspsr_optim_workspace_bytes() // 4, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()

    def optim(kind, b, a2, r):
        return lambda: lib.jspsr_optim_step(kind, P(p), P(g), P(s1), None if kind == 0 else P(s2), N_PARAMS, 1e-6, 0.9, a2, 1e-8, 1e-6,
                                            5, None, P(rng) if r else None, P(ws) if r else None, stream)

    legs = [("jspsr_adamw_step (baseline)", 28, lambda: lib.jspsr_adamw_step(P(p), P(g), P(s1), P(s2), N_PARAMS, 1e-6, 0.9, 0.999,
                                                                              1e-8, 1e-6, 5, stream))]
    for label, kind, b, a2 in (("AdamW", 2, 28, 0.999), ("SGD momentum", 0, 20, 0.0), ("Adam", 1, 28, 0.999),
                               ("RMSprop momentum", 3, 28, 0.99)):
        legs.append((f"jspsr_optim_step {label}", b, optim(kind, b, a2, False)))
        legs.append((f"jspsr_optim_step {label} + range", b, optim(kind, b, a2, True)))
    for _, _, fn in legs:                       # warm-up: code objects, clocks
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in legs}
    for _ in range(reps):
        for name, _, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    out.append(f"1. step kernels at {N_PARAMS} parameters (us per launch, device events around {iters} launches, {reps} repetitions, "
               "legs alternating)")
    for name, b, _ in legs:
        med, text = line(times[name], "us")
        out.append(f"   {name:44s} {text}   {b} B/param -> {b * N_PARAMS / med / 1e6:7.2f} TB/s")


def grad_range_reference(model):
    """get_gradient_range (train/train_utils.py:127-143) as written there."""
    lo, hi = 999, -999
    for _, param in model.named_parameters():
        if param.grad is not None:
            lo = min(lo, param.grad.min())
            hi = max(hi, param.grad.max())
    return [lo, hi]


def epoch_wall_time(reps, steps, nf, out):
    from jspsr_amd.JSPSR import Model
    dev = "cuda:0"
    m = Model(dict(IC, COP30=1), num_feature=nf)
    m.load_state_dict(R.make_state_dict(R.jspsr_param_shapes(IC, nf), seed=5))
    m = m.to(dev).train()
    m.compute_dtype = torch.bfloat16
    red = GradReducer(m.parameters())
    red.watch_streams(m.side_streams("cuda"))
    opt = O.FlatAdamW(red, lr=1e-4, weight_decay=1e-6)
    sch = O.ConstantLR(opt)
    crit = L.get_criterion({"L1": 1.0, "L2": 1.0, "Grad": 0.1})
    inputs, gt = R.synthetic_batch(8, 512, 512, True, seed=6)
    batch = {"lr_dem": inputs[0].to(dev), "image": inputs[1].to(dev), "mask": inputs[2].to(dev), "hr_dem": gt.to(dev), "base": None,
             "meta": [None] * 8}
    batches = [batch] * steps

    def leg_a(monitor):
        return lambda: TR.train_one_epoch(m, batches, crit, opt, sch, red, "JSPSR", IC, monitor_value=monitor)

    def leg_b(with_range):
        def run():
            m.train()
            mon = TR.LossMonitor(["L1", "L2", "Grad", "Total"])
            for b in batches:
                crit.reset()
                inp, target, _, _ = TR.batch_pair(b, "JSPSR", IC)
                red.zero_grad()
                res = crit(m(*inp), target)
                res["Total"].backward()
                red.finish()
                opt.step()
                mon.update({k: v.item() for k, v in res.items()}, target.size(0))
                if with_range:
                    r = grad_range_reference(m)
                    "({:6.4f} {:6.4f})".format(r[0], r[1])
            sch.step()
            return mon.avg["Total"]
        return run

    legs = [("A  train_one_epoch", leg_a(())), ("A  train_one_epoch, monitor grad", leg_a(("grad",))),
            ("B  loop with 4 .item() per step", leg_b(False)), ("C  B + per-parameter gradient range", leg_b(True))]
    leg_a(())()                                 # warm-up of every shape: two short epochs
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
    out.append(f"2. epoch of {steps} steps, JSPSR nf {nf} image + mask, 8 x 512 x 512 bf16 (ms per step, host clock around an epoch "
               f"ending in a synchronise, {reps} repetitions, legs alternating)")
    med = {}
    for name, _ in legs:
        med[name], text = line(times[name], "ms")
        out.append(f"   {name:44s} {text}")
    a, ag, b, c = (med[name] for name, _ in legs)
    out.append(f"   B / A = {b / a:.3f}    C / A(monitor grad) = {c / ag:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--nf", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_epoch_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epoch.py measures on the GPU only")
    out = [f"tools/bench_epoch.py on {torch.cuda.get_device_name(0)}, host CPUs visible: {os.cpu_count()}, torch {torch.__version__}"]
    kernel_bandwidth(args.reps, args.iters, out)
    epoch_wall_time(args.reps, args.steps, args.nf, out)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
