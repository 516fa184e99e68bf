"""K1p micro-benchmark: the plain 3x3 one-channel head (jspsr_conv_head1_*) against the generic conv route (ops._Conv) on
the same shape, plus one informational eager training step of each plain-head model.
Usage: python tools/bench_head1.py [B H W C]        (default 8 512 512 64)

Algorithmic bytes per pixel: forward C s + 4, backward 2 C s + 4 (s = element size of the compute dtype).  300 launches of
warm-up before timing (the clocks settle), and the operand sets rotate past the 256 MB Infinity Cache."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jspsr_amd import _lib, ops  # noqa: E402
from jspsr_amd import kernels as K  # noqa: E402

PEAK = 8.0e12   # MI355X HBM3E, bytes/s


def _time(fn, nset, warm=300, iters=100):
    for i in range(warm):
        fn(i % nset)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % nset)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def kernel_rows(B, H, W, C, dtype):
    lib = _lib.load()
    s = torch.tensor([], dtype=dtype).element_size()
    npx = B * H * W
    nset = max(2, int(600e6 // (npx * (2 * C * s + 8))) + 1)
    g = torch.Generator(device="cuda").manual_seed(0)
    xs = [torch.randn(B, H, W, C, device="cuda", generator=g).to(dtype) for _ in range(nset)]
    dxs = [torch.empty_like(x) for x in xs]
    dys = [torch.randn(B, 1, H, W, device="cuda", generator=g) for _ in range(nset)]
    w = torch.randn(1, C, 3, 3, device="cuda", generator=g) * 0.05
    b = torch.zeros(1, device="cuda")
    y = torch.empty(B, 1, H, W, device="cuda")
    dw, db = torch.empty_like(w), torch.empty_like(b)
    ws = torch.empty(lib.jspsr_conv_head1_workspace_bytes(B, H, W, C), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dt = K._dt(xs[0])

    def fwd(i):
        lib.jspsr_conv_head1_forward(dt, xs[i].data_ptr(), C, 0, C, w.data_ptr(), b.data_ptr(), y.data_ptr(), B, H, W, st)

    def bwd(i):
        lib.jspsr_conv_head1_backward(dt, dys[i].data_ptr(), xs[i].data_ptr(), C, 0, C, w.data_ptr(), dxs[i].data_ptr(), C, 0,
                                      dw.data_ptr(), db.data_ptr(), ws.data_ptr(), B, H, W, st)

    fwd(0); bwd(0)
    _lib.check(0, "warm")
    t_f, t_b = _time(fwd, nset), _time(bwd, nset)
    fb, bb = npx * (C * s + 4), npx * (2 * C * s + 4)
    # the generic route: ops._Conv forward (bf16 / fp32 output, NHWC) + backward (dx, dW, db), and the NHWC -> NCHW pass
    wp = torch.nn.Parameter(w.clone())
    bp = torch.nn.Parameter(b.clone())
    xg = [x.detach().requires_grad_() for x in xs]

    def gen_fwd(i):
        with torch.no_grad():
            ops.conv2d(xs[i], wp, bp, 1, 1).float().reshape(B, 1, H, W)

    def gen_fb(i):
        out = ops.conv2d(xg[i], wp, bp, 1, 1).float().reshape(B, 1, H, W)
        torch.autograd.grad(out, (xg[i], wp, bp), dys[i])

    t_gf = _time(gen_fwd, nset, warm=50, iters=30)
    t_gfb = _time(gen_fb, nset, warm=50, iters=30)
    name = "bf16" if dtype == torch.bfloat16 else "fp32"
    return {"shape": [B, H, W, C], "dtype": name,
            "head1_fwd_us": round(t_f, 1), "head1_fwd_GBps": round(fb / t_f / 1e3), "head1_fwd_frac_8TBps": round(fb / t_f / 1e-6 / PEAK, 3),
            "head1_bwd_us": round(t_b, 1), "head1_bwd_GBps": round(bb / t_b / 1e3), "head1_bwd_frac_8TBps": round(bb / t_b / 1e-6 / PEAK, 3),
            "generic_fwd_us": round(t_gf, 1), "generic_bwd_us": round(t_gfb - t_gf, 1), "operand_sets": nset}


def step_row(name, dtype, B=8, H=512, W=512):
    from jspsr_amd.EDSR import EDSR
    from jspsr_amd.JSPSR import Model
    from jspsr_amd.losses import MultiLoss
    from oracle import jspsr_ref as R
    if name == "jspsr":
        m = Model({"lr_dem": 1, "image": 3, "mask": 15, "COP30": 1}, num_feature=32, spn=False)
    else:
        m = EDSR(in_channels=4, out_channels=1, n_resblocks=16, n_features=64, scale=1)
    m = m.cuda().train()
    m.compute_dtype = dtype
    inputs, gt = R.synthetic_batch(B, H, W, name == "jspsr", seed=1)
    inputs, gt = [t.cuda() for t in inputs], gt.cuda()
    args = inputs if name == "jspsr" else [torch.cat(inputs[:2], 1)]
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
    crit = MultiLoss(1.0, 1.0, 0.1)

    def one():
        m.zero_grad(set_to_none=True)
        crit(m(*args), gt)["Total"].backward()
        opt.step()

    for _ in range(5):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        one()
    torch.cuda.synchronize()
    return {"model": name + "(spn=False)", "config": [B, H, W], "dtype": "bf16" if dtype == torch.bfloat16 else "fp32",
            "eager_step_ms": round((time.perf_counter() - t0) / 10 * 1e3, 2)}


def main():
    a = [int(v) for v in sys.argv[1:5]] if len(sys.argv) >= 5 else [8, 512, 512, 64]
    print(f"# {torch.cuda.get_device_name(0)}", flush=True)
    for dtype in (torch.bfloat16, torch.float32):
        print(json.dumps(kernel_rows(*a, dtype)), flush=True)
    for name in ("jspsr", "edsr"):
        print(json.dumps(step_row(name, torch.bfloat16)), flush=True)


if __name__ == "__main__":
    main()
