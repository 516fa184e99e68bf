"""K9 batch micro-benchmark (csrc/batch.hip, jspsr_amd/data.py) at the configs' training shape: B x k^2 crops of 334^2
scenes with image (3) + mask (15), log-scaled relative DEMs (configs/jspsr_r3_img_msk.yml).  Legs, in one process:
  * the jspsr_batch_make launch alone, on a table already on the device (device events around `iters` launches);
  * one RandomCropBatches epoch end to end (host draws + one table upload + a launch per batch; host clock around the
    epoch, ended by a synchronise);
  * the reference's per-sample host chain restated in numpy (RandomCrop -> RandomFlipRotate90 -> ToTensor,
    tests/batches_ref.py) and the stacking of a batch (np.stack + torch.from_numpy), on one CPU core.
Bytes per batch from the shapes: every source byte of the crops read once, every fp32 output written once.  The ceiling is
the 6.3 TB/s a device-to-device copy reaches (MI355X_MICROARCH.md), not the 8 TB/s HBM peak.
Usage: python tools/bench_batches.py [B k] [--scenes N]         (default 50 128, 64 scenes)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jspsr_amd import _lib  # noqa: E402
from jspsr_amd import data as D  # noqa: E402
from tests import batches_ref as R  # noqa: E402

COPY_CEIL = 6.3e12
P = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True, scale_mask=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B, k = (int(args[0]), int(args[1])) if len(args) >= 2 else (50, 128)
    n_sc = int(sys.argv[sys.argv.index("--scenes") + 1]) if "--scenes" in sys.argv else 64
    assert torch.cuda.is_available(), "bench_batches needs the MI355X"
    _lib.load()
    scenes = R.make_scenes([(334, 334)] * n_sc, seed=1)
    for s in scenes:
        del s["canopy"]
    S = D.DeviceScenes(**{kk: [s[kk] for s in scenes] for kk in ("lr_dem", "hr_dem", "image", "mask")}, device="cuda", **P)
    bytes_px = sum(S.channels[kk] * (4 if "dem" in kk else 1) for kk in S.kinds) + 4 * sum(S.channels[kk] for kk in S.kinds)
    nbytes = B * k * k * bytes_px

    # the launch alone
    it = D.RandomCropBatches(S, B, k, rng=np.random.RandomState(0), sampler=list(range(n_sc)) * ((B + n_sc - 1) // n_sc))
    rows, sides, metas = it.draw(list(it.sampler)[:B])
    table = torch.from_numpy(rows).to("cuda")
    outs = {kk: (torch.empty((B, S.channels[kk], k, k), device="cuda"), 0) for kk in S.kinds}
    for _ in range(30):
        S.make(table, k, outs)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters = 400
    e0.record()
    for _ in range(iters):
        S.make(table, k, outs)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3

    # one epoch end to end (host draws + upload + launches), 20 batches
    sampler = list(range(n_sc)) * ((20 * B + n_sc - 1) // n_sc)
    ep = D.RandomCropBatches(S, B, k, rng=np.random.RandomState(1), sampler=sampler[:20 * B])
    list(ep)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for batch in ep:
        pass
    host_only = time.perf_counter() - t0
    torch.cuda.synchronize()
    epoch_us = (time.perf_counter() - t0) / 20 * 1e6

    # the reference's per-sample chain on the host, in numpy (one core)
    torch.set_num_threads(1)
    rs = np.random.RandomState(2)
    p = dict(R.PARAMS, **P)
    host = [dict(s) for s in scenes[:8]]
    n = 100
    t0 = time.perf_counter()
    samples = []
    for j in range(n):
        sc = host[j % len(host)]
        crop, aug = R.draw(rs, 334, 334, k)
        samples.append(R.sample(sc, p, k, crop, aug)[0])
    per_sample = (time.perf_counter() - t0) / n
    t0 = time.perf_counter()
    sb = samples[:B] if len(samples) >= B else (samples * ((B + len(samples) - 1) // len(samples)))[:B]
    {kk: torch.from_numpy(np.stack([s[kk] for s in sb])) for kk in sb[0]}
    stack_s = time.perf_counter() - t0

    res = {"kernel": "jspsr_batch_make", "B": B, "k": k, "kinds": S.kinds, "channels": S.channels,
           "bytes_per_batch": nbytes, "us_per_batch": round(us, 2), "GBps": round(nbytes / us * 1e-3, 1),
           "fraction_of_copy_ceiling": round(nbytes / (us * 1e-6) / COPY_CEIL, 3),
           "epoch_us_per_batch": round(epoch_us, 1), "epoch_host_enqueue_us_per_batch": round(host_only / 20 * 1e6, 1),
           "host_chain_ms_per_sample": round(per_sample * 1e3, 3), "host_chain_samples_per_s_one_core": round(1 / per_sample, 1),
           "host_stack_ms_per_batch": round(stack_s * 1e3, 2),
           "host_one_core_ms_per_batch": round((per_sample * B + stack_s) * 1e3, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
