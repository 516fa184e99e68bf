"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/g9_*.npz: the plain-head models (JSPSR spn=False, EDSR spn=False)
made by the reference's own modules, as oracle/gen_golden.py does for the spn=True models.

Run where the reference tree is available (never on the GPU box):

    python tools/gen_golden_plain.py [name-filter ...]

Parameters and inputs come from numpy's frozen legacy RandomState stream (oracle.jspsr_ref.make_state_dict /
synthetic_batch); the fixtures store the seed and checksums, so the tests regenerate them and fail on a mismatch.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import jspsr_ref as R  # noqa: E402
from oracle.gen_golden import import_reference  # noqa: E402
from tests import plain_head_ref as P  # noqa: E402

IMG = {"lr_dem": 1, "image": 3}
MSK = {"lr_dem": 1, "image": 3, "mask": 15}


def _common(store, sd, inputs, gt, seed, B, H, W, training, model):
    store.update({"seed": np.int64(seed), "BHW": np.array([B, H, W]), "training": np.bool_(training),
                  "param_checksum": np.float64(R.checksum(sd.values())),
                  "input_checksum": np.float64(R.checksum(list(inputs) + [gt])),
                  "sd_keys": np.array(list(model.state_dict())),
                  "sd_shapes": np.array([str(tuple(v.shape)) for v in model.state_dict().values()])})


def _grads(model, store, save):
    names, norms = [], []
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        names.append(k)
        norms.append(p.grad.norm().item())
        if k in save:
            store["grad:" + k] = p.grad.numpy()
    store["grad_names"] = np.array(names)
    store["grad_norms"] = np.array(norms)


def gen_jspsr(ref_jspsr, path, in_channels, nf, B, H, W, seed, training):
    shapes = P.jspsr_plain_param_shapes(in_channels, nf)
    sd = R.make_state_dict(shapes, seed, torch.float64)
    np.random.seed(0)
    model = ref_jspsr.Model(in_channels=dict(in_channels, COP30=1), out_channels=1, num_feature=nf,
                            layers=(2, 2, 2, 2), spn=False)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == list(shapes.items()), "param table != reference"
    model = model.double()
    model.load_state_dict(sd, strict=True)
    model.train(training)
    inputs, gt = R.synthetic_batch(B, H, W, "mask" in in_channels, seed=seed + 1, dtype=torch.float64)
    pred = model(*inputs)
    loss = (pred - gt).abs().mean() + ((pred - gt) ** 2).mean()
    # the helper restatement must agree with the reference modules before anything is stored
    sd_chk = {k: v.clone() for k, v in sd.items()}
    ref_pred = P.jspsr_plain_forward(sd_chk, inputs, training)
    assert (ref_pred - pred.detach()).abs().max().item() < 1e-10, "tests/plain_head_ref.py != reference"
    store = {"pred": pred.detach().numpy(), "loss": np.float64(loss.item()), "nf": np.int64(nf)}
    _common(store, sd, inputs, gt, seed, B, H, W, training, model)
    if training:
        (pred * R.probe_gradient(pred.shape, seed + 2)).mean().backward()
        # conv0's weight (the layer feeding the head) only where it is small: at nf 32 it alone is 1.2 MB
        big = nf > 8
        _grads(model, store, ("postprocessor.conv.0.weight", "postprocessor.conv.0.bias", "conv0.conv.bn.weight",
                              "conv0.conv.bn.bias", "conv_dem.conv.0.weight") + (() if big else ("conv0.conv.0.weight",)))
        new_sd = model.state_dict()
        for k in ("conv_img.conv.bn.running_mean", "layer3_dem.0.bn1.running_var", "conv0.conv.bn.running_mean"):
            store["buf:" + k] = new_sd[k].numpy()
    model32 = ref_jspsr.Model(in_channels=dict(in_channels, COP30=1), num_feature=nf, spn=False).float()
    model32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()})
    model32.train(training)
    with torch.no_grad():
        store["pred_fp32"] = model32(*[t.float() for t in inputs]).numpy()
    np.savez(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def gen_edsr(path, B, H, W, seed, training, n_resblocks=4, n_features=32):
    import models.EDSR as ref_edsr
    shapes = P.edsr_plain_param_shapes(4, n_resblocks, n_features)
    sd = R.make_state_dict(shapes, seed, torch.float64)
    model = ref_edsr.EDSR(in_channels=4, out_channels=1, n_resblocks=n_resblocks, n_features=n_features, scale=1)
    assert not model.spn      # the factory's default for EDSR (utils/config.py:95-99)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == list(shapes.items()), "param table != reference"
    model = model.double()
    model.load_state_dict(sd, strict=True)
    model.train(training)
    inputs, gt = R.synthetic_batch(B, H, W, False, seed=seed + 1, dtype=torch.float64)
    x = torch.cat(inputs, 1)
    pred = model(x)
    ref_pred = P.edsr_plain_forward(sd, x, training, n_resblocks)
    assert (ref_pred - pred.detach()).abs().max().item() < 1e-10, "tests/plain_head_ref.py != reference"
    loss = ((pred - gt) ** 2).mean()
    store = {"pred": pred.detach().numpy(), "loss": np.float64(loss.item()), "n_resblocks": np.int64(n_resblocks),
             "n_features": np.int64(n_features)}
    _common(store, sd, inputs, gt, seed, B, H, W, training, model)
    if training:
        (pred * R.probe_gradient(pred.shape, seed + 2)).mean().backward()
        _grads(model, store, ("entry.weight", f"encoder.{n_resblocks}.weight", "head.weight", "head.bias"))
    model32 = ref_edsr.EDSR(in_channels=4, out_channels=1, n_resblocks=n_resblocks, n_features=n_features, scale=1).float()
    model32.load_state_dict({k: v.float() for k, v in sd.items()})
    with torch.no_grad():
        store["pred_fp32"] = model32(x.float()).numpy()
    np.savez(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def gen_init_stream(ref_jspsr, path, in_channels, nf, seed):
    """The reference's `_initialize_weights` (models/JSPSR.py:494-517) for spn=False under np.random.seed(seed), compared
    bit for bit with the port's, and summarised per tensor (sum / abs-sum / first / last) for the box without it."""
    from jspsr_amd.JSPSR import Model
    np.random.seed(seed)
    ref = ref_jspsr.Model(in_channels=dict(in_channels, COP30=1), out_channels=1, num_feature=nf,
                          layers=(2, 2, 2, 2), spn=False).state_dict()
    np.random.seed(seed)
    mine = Model(dict(in_channels, COP30=1), num_feature=nf, spn=False).state_dict()
    assert list(ref) == list(mine), "state_dict key order differs"
    for k in ref:
        assert ref[k].dtype == mine[k].dtype and torch.equal(ref[k], mine[k]), f"init stream differs at {k}"
    names = list(ref)
    summ = np.zeros((len(names), 4))
    for i, k in enumerate(names):
        t = ref[k].double().reshape(-1)
        summ[i] = (t.sum().item(), t.abs().sum().item(), t[0].item(), t[-1].item())
    np.savez(path, names=np.array(names), summary=summ, seed=np.int64(seed), nf=np.int64(nf),
             with_mask=np.bool_("mask" in in_channels))
    print("wrote", path, os.path.getsize(path) // 1024, "KiB (reference init == product init,", len(names), "tensors)")


def main():
    ref_jspsr, _ = import_reference()
    out = os.path.join(REPO, "tests", "golden")
    only = set(sys.argv[1:])

    def want(name):
        return not only or any(o in name for o in only)

    jobs = [
        ("g9_jspsr_img_nf8_b2_48x64_train.npz", lambda p: gen_jspsr(ref_jspsr, p, IMG, 8, 2, 48, 64, 91, True)),
        ("g9_jspsr_msk_nf8_b2_64_eval.npz", lambda p: gen_jspsr(ref_jspsr, p, MSK, 8, 2, 64, 64, 92, False)),
        ("g9_jspsr_msk_nf32_b1_64_train.npz", lambda p: gen_jspsr(ref_jspsr, p, MSK, 32, 1, 64, 64, 93, True)),
        ("g9_init_stream_msk_nf8.npz", lambda p: gen_init_stream(ref_jspsr, p, MSK, 8, 94)),
        ("g9_edsr_b2_40x56_train.npz", lambda p: gen_edsr(p, 2, 40, 56, 95, True)),
    ]
    for name, fn in jobs:
        if want(name):
            fn(os.path.join(out, name))


if __name__ == "__main__":
    main()
