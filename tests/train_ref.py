"""TEST INFRASTRUCTURE ONLY -- what tools/gen_golden_train.py and the training-loop tests share: the seeded small model
and batches of fixture g13 (b), the configurations of its schedules (a), the scripted curves of the EarlyStopper
decisions (c), and a torch restatement of kornia's spatial_gradient (sobel, normalised, replicate padding -- from
kornia's public documentation) that stands in for the package while the reference's EdgeLoss runs in the generator.

Everything random comes from numpy's legacy RandomState stream (frozen by NEP 19); the fixture stores the seed and a
checksum of the regenerated inputs, and the tests fail on a mismatch."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

SEED = 1307
OPTIMIZERS = ("SGD", "Adam", "AdamW", "RMSprop")
SCHEDULERS = ("OneCycleLR", "CosineAnnealingLR", "StepLR", "WarmupStepLR", "ConstantLR")
SCHEDULE_EPOCHS = (12, 300)
OPT_KW = {"lr": 1e-3, "momentum": 0.9, "weight_decay": 1e-6}
SCHED_KW = {"warmup_epoch": 3, "max_lr": 0.01}
# (b): two epochs of six steps (five batches of 4, one of 3), the reference's MultiLoss weights, a schedule that moves
LOSS = {"L1": 1.0, "L2": 1.0, "Grad": 0.1}
EPOCH_OPT_KW = {"SGD": {"lr": 1e-2, "momentum": 0.9, "weight_decay": 1e-6}, "Adam": {"lr": 1e-3, "momentum": 0.9, "weight_decay": 1e-6},
                "AdamW": {"lr": 1e-3, "momentum": 0.9, "weight_decay": 1e-6}, "RMSprop": {"lr": 1e-3, "momentum": 0.9, "weight_decay": 1e-6}}
EPOCH_SCHEDULER, EPOCH_EPOCHS, EPOCHS_RUN = "CosineAnnealingLR", 4, 2
BATCH_SIZES = (4, 4, 4, 4, 4, 3)
SIDE = 16
INPUT_DATA = {"lr_dem": 1, "image": 3}
MONITORS = ("val_loss", "trainval_loss", "val_psnr", "val_ssim", "val_rmse")
CURVES = ("improving", "plateau", "noisy")
PATIENCE, MIN_DELTA = 3, 1e-4


class SmallNet(torch.nn.Module):
    """Three Conv2d on lr_dem + image, residual on lr_dem; the last one is named `postprocessor` so that the reference's
    diff_lr grouping (named parameters containing "postprocessor") finds a second group."""

    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(4, 6, 3, padding=1)
        self.conv2 = torch.nn.Conv2d(6, 6, 3, padding=1)
        self.postprocessor = torch.nn.Conv2d(6, 1, 3, padding=1)

    def forward(self, lr_dem, image):
        x = torch.relu(self.conv1(torch.cat((lr_dem, image), 1)))
        x = torch.relu(self.conv2(x))
        return lr_dem + self.postprocessor(x)


def small_net(seed=SEED):
    net = SmallNet()
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.from_numpy(rs.standard_normal(tuple(p.shape)) * (0.15 if p.dim() == 4 else 0.02)).float())
    return net


def batches(seed=SEED + 1):
    """The epoch's batches: dicts as data.RandomCropBatches yields them (CPU tensors)."""
    rs = np.random.RandomState(seed)
    out = []
    for k, b in enumerate(BATCH_SIZES):
        coarse = torch.from_numpy(rs.uniform(0.2, 0.8, (b, 1, 4, 4)))
        lr = F.interpolate(coarse, size=(SIDE, SIDE), mode="bilinear", align_corners=True)
        hr = lr + torch.from_numpy(rs.standard_normal((b, 1, SIDE, SIDE)) * 0.03)
        img = torch.from_numpy(rs.uniform(0.0, 1.0, (b, 3, SIDE, SIDE)))
        out.append({"lr_dem": lr.float(), "image": img.float(), "hr_dem": hr.float(), "base": torch.zeros(b),
                    "meta": [{"id": f"g13-{k}-{j}"} for j in range(b)]})
    return out


def checksum(tensors):
    return float(sum(float(np.abs(np.asarray(t, dtype=np.float64)).sum()) for t in tensors))


def inputs_checksum():
    net, bs = small_net(), batches()
    return checksum([p.detach().numpy() for p in net.parameters()] + [b[k].numpy() for b in bs for k in ("lr_dem", "image", "hr_dem")])


def spatial_gradient(x):
    """kornia.filters.spatial_gradient(x, mode="sobel", order=1, normalized=True): (B,C,H,W) -> (B,C,2,H,W), the Sobel pair
    divided by 8 over a replicate-padded input, as cross-correlations."""
    b, c, h, w = x.shape
    kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=x.dtype, device=x.device) / 8.0
    k = torch.stack((kx, kx.t())).unsqueeze(1)
    y = F.conv2d(F.pad(x.reshape(b * c, 1, h, w), (1, 1, 1, 1), mode="replicate"), k)
    return y.view(b, c, 2, h, w)


def schedule_key(scheduler, optimizer, diff_lr, epochs):
    return f"sch_{scheduler}_{optimizer}_{'diff' if diff_lr else 'one'}_{epochs}"


def curve(name, n=14):
    """A scripted validation history: n rows of (val_loss, train_loss, {"PSNR", "SSIM", "RMSE"}).
    improving: everything gets better; plateau: improves, then stalls within min_delta; noisy: the loss wanders upwards
    while PSNR / SSIM keep improving and the RMSE stalls (so the monitored score and the loss disagree)."""
    rs = np.random.RandomState(SEED + 2 + CURVES.index(name))
    rows = []
    for e in range(n):
        if name == "improving":
            val, train = 1.0 / (e + 2), 0.9 / (e + 2)
            psnr, ssim, rmse = 20.0 + e, 0.5 + 0.03 * e, 3.0 / (e + 1)
        elif name == "plateau":
            f = min(e, 5)
            val, train = 0.5 - 0.05 * f + (2e-5 * (e % 2) if e > 5 else 0.0), 0.6 - 0.05 * f
            psnr, ssim, rmse = 25.0 + f, 0.6 + 0.02 * f, 2.0 - 0.1 * f + (3e-5 if e > 5 else 0.0)
        else:
            val, train = 0.3 + 0.01 * e + 0.02 * float(rs.standard_normal()), 0.31 + 0.008 * e
            psnr, ssim, rmse = 22.0 + 0.5 * e, 0.55 + 0.01 * e, 1.5 + (0.0 if e < 4 else 0.01 * (e % 3))
        rows.append((float(val), float(train), {"PSNR": float(psnr), "SSIM": float(ssim), "RMSE": float(rmse)}))
    return rows


def decisions(stopper, rows):
    return [bool(stopper(v, t, dict(s))) for v, t, s in rows]
