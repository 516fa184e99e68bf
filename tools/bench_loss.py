"""Loss-menu micro-benchmark (csrc/loss_terms.hip) at B x 1 x H x W fp32, all legs in one process:
  * the default MultiLoss(1, 1, 0.1) (jspsr_loss_forward / _backward),
  * SSIM forward and backward alone (jspsr_loss_menu_forward / _backward, terms = SSIM),
  * the pointwise terms BerHu + BCE + Norm together,
  * the 5-term criterion {L1: 1, L2: 1, Grad: 0.1, SSIM: 0.5, Berhu: 0.2} (get_criterion), forward + backward,
  * the same 5 terms as a torch-operator composition on the GPU (comparison only; BerHu's threshold kept on the device),
  * one eager nf 32 JSPSR training step with the 5-term criterion and with MultiLoss(1, 1, 0.1), alternated.
Usage: python tools/bench_loss.py [B H W] [--no-step]      (default 8 512 512)

SSIM bounds (from the shapes): forward 5 moments x 22 separable taps x 2 FLOP per map element, bytes = pred + gt read
+ alpha, beta, gamma written; backward 3 maps x 22 taps x 2 FLOP per pixel, bytes = alpha, beta, gamma + pred + gt read,
the gradient read and written.  Peaks: 157.3 TFLOP/s fp32 vector, 8.0 TB/s HBM."""
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jspsr_amd import _lib  # noqa: E402
from jspsr_amd.losses import MultiLoss, get_criterion  # noqa: E402

PEAK_BW, PEAK_FP32 = 8.0e12, 157.3e12
FIVE = {"L1": 1, "L2": 1, "Grad": 0.1, "SSIM": 0.5, "Berhu": 0.2}


def _time(fn, warm=30, iters=100):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def _torch_five(pred, gt):
    """The 5 terms as torch operators (replicate-padded normalised Sobel, valid Gaussian SSIM, device-side BerHu)."""
    d = pred - gt
    l1, l2 = d.abs().mean(), (d * d).mean()
    kx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], device=pred.device) / 8
    k = torch.stack((kx, kx.t())).unsqueeze(1)
    grad = F.conv2d(F.pad(d, (1, 1, 1, 1), mode="replicate"), k).abs().mean()
    c = torch.arange(11, dtype=torch.float32, device=pred.device) - 5
    w = torch.exp(-c * c / 4.5)
    w = w / w.sum()
    wx, wy = w.view(1, 1, 1, 11), w.view(1, 1, 11, 1)
    x = pred.clamp(0, 1)

    def filt(t):
        return F.conv2d(F.conv2d(t, wx), wy)
    mx, my = filt(x), filt(gt)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(gt * gt) - my * my, filt(x * gt) - mx * my
    s = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    ssim = 1 - s.mean()
    ad = d.abs()
    th = 0.6 * ad.max().detach()
    berhu = torch.where(ad <= th, ad, (ad * ad + th * th) / (2 * th)).mean()
    return l1 + l2 + 0.1 * grad + 0.5 * ssim + 0.2 * berhu


def kernel_rows(B, H, W):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    gt = torch.rand(B, 1, H, W, device="cuda", generator=g) * 0.8 + 0.1
    pred = (gt + 0.05 * torch.randn(B, 1, H, W, device="cuda", generator=g)).contiguous()
    out = {"shape": [B, 1, H, W]}

    x = pred.clone().requires_grad_()
    ml = MultiLoss(1, 1, 0.1)
    out["multiloss_fwd_us"] = round(_time(lambda: ml(x, gt)), 1)
    out["multiloss_fwd_bwd_us"] = round(_time(lambda: ml(x, gt)["Total"].backward()), 1)

    def raw(terms, slots):
        n = len(slots)
        ws = torch.empty(lib.jspsr_loss_menu_workspace_bytes(terms, B, H, W), dtype=torch.uint8, device="cuda")
        o = torch.empty(n + 1, device="cuda")
        gp = torch.zeros_like(pred)
        cs, cw = (ctypes.c_int * n)(*slots), (ctypes.c_double * n)(*[1.0] * n)
        sw = (ctypes.c_double * 7)(*[1.0] * 7)
        fwd = lambda: lib.jspsr_loss_menu_forward(pred.data_ptr(), gt.data_ptr(), terms, B, H, W, n, cs, cw, None,  # noqa: E731
                                                  o.data_ptr(), ws.data_ptr(), st)
        bwd = lambda: lib.jspsr_loss_menu_backward(pred.data_ptr(), gt.data_ptr(), terms, B, H, W, sw, None,  # noqa: E731
                                                   gp.data_ptr(), ws.data_ptr(), st)
        assert fwd() == 0 and bwd() == 0
        return _time(fwd), _time(bwd)

    f, b = raw(8, [6])
    M, N = B * (H - 10) * (W - 10), B * H * W
    fl_f, by_f = M * 5 * 22 * 2, 2 * N * 4 + 3 * M * 4
    fl_b, by_b = N * 3 * 22 * 2, 3 * M * 4 + 4 * N * 4
    for tag, t, fl, by in (("fwd", f, fl_f, by_f), ("bwd", b, fl_b, by_b)):
        tb, tf = by / PEAK_BW * 1e6, fl / PEAK_FP32 * 1e6
        out[f"ssim_{tag}_us"] = round(t, 1)
        out[f"ssim_{tag}_bound"] = "bytes" if tb >= tf else "flops"
        out[f"ssim_{tag}_share_of_bound"] = round(max(tb, tf) / t, 3)
        out[f"ssim_{tag}_GBps"] = round(by / t / 1e3)
    f, b = raw(1 | 2 | 4, [3, 4, 5])
    out["pointwise_fwd_us"], out["pointwise_bwd_us"] = round(f, 1), round(b, 1)

    crit = get_criterion(FIVE)
    out["five_fwd_us"] = round(_time(lambda: crit(x, gt)), 1)
    out["five_fwd_bwd_us"] = round(_time(lambda: crit(x, gt)["Total"].backward()), 1)
    out["five_over_multiloss"] = round(out["five_fwd_bwd_us"] / out["multiloss_fwd_bwd_us"], 2)
    out["torch_five_fwd_bwd_us"] = round(_time(lambda: _torch_five(x, gt).backward()), 1)
    out["targets"] = {"ssim_fwd_le_30us": out["ssim_fwd_us"] <= 30, "ssim_bwd_le_60us": out["ssim_bwd_us"] <= 60,
                      "five_le_3x_multiloss": out["five_over_multiloss"] <= 3}
    return out


def step_rows(B, H, W, nf=32, reps=5, iters=10):
    """Eager training steps, the two criteria alternated in `reps` rounds of `iters` steps; medians of the rounds."""
    from jspsr_amd.ddp import GradReducer
    from jspsr_amd.JSPSR import Model
    from jspsr_amd.optim import FlatAdamW
    from oracle import jspsr_ref as R
    ic = {"lr_dem": 1, "image": 3, "mask": 15}
    m = Model(dict(ic, COP30=1), num_feature=nf)
    m.load_state_dict(R.make_state_dict(R.jspsr_param_shapes(ic, nf), seed=5))
    m = m.cuda().train()
    red = GradReducer(m.parameters())
    if hasattr(m, "side_streams"):
        red.watch_streams(m.side_streams("cuda"))
    opt = FlatAdamW(red, lr=1e-5, weight_decay=1e-6)
    inputs, gt = R.synthetic_batch(B, H, W, True, seed=6)
    inputs, gt = [t.cuda() for t in inputs], gt.cuda()
    crits = {"multiloss": MultiLoss(1, 1, 0.1), "five": get_criterion(FIVE)}

    def step(c):
        red.zero_grad()
        c(m(*inputs), gt)["Total"].backward()
        red.finish()
        opt.step()
    times = {k: [] for k in crits}
    for k, c in crits.items():
        for _ in range(3):
            step(c)
    for _ in range(reps):
        for k, c in crits.items():
            times[k].append(_time(lambda: step(c), warm=1, iters=iters) / 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return {"model": f"jspsr nf{nf}", "config": [B, H, W], "step_ms_multiloss": round(med["multiloss"], 3),
            "step_ms_five": round(med["five"], 3), "delta_ms": round(med["five"] - med["multiloss"], 3),
            "rounds_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
            "target_delta_le_0.3ms": med["five"] - med["multiloss"] <= 0.3}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B, H, W = (int(a) for a in args) if args else (8, 512, 512)
    assert torch.cuda.is_available(), "bench_loss needs the GPU"
    print(f"# {torch.cuda.get_device_name(0)}")
    print(json.dumps(kernel_rows(B, H, W)))
    if "--no-step" not in sys.argv:
        print(json.dumps(step_rows(B, H, W)))


if __name__ == "__main__":
    main()
