"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/g13_train.npz: the training loop's numbers made by the reference's
own code (utils.common_config get_optimizer / get_scheduler / get_criterion, train.train_utils train_one_epoch /
EarlyStopper), imported as tools/gen_golden_eval.py does: placeholder modules for the packages this image lacks, a
dict with attribute access for easydict, and tests/train_ref.py:spatial_gradient for kornia's (EdgeLoss).
`get_batch_pair` moves its tensors to a GPU; a stand-in that returns the same lists from CPU tensors replaces it.

Run where the reference tree is available (never on the GPU box):

    python tools/gen_golden_train.py

The fixture holds data only: arrays, and JSON strings of settings and names.
 (a) schedules: per-epoch lr and momentum / betas[0] of every group for scheduler x optimizer x diff_lr x epochs;
 (b) two epochs of train_one_epoch on tests/train_ref.py's small model for each optimizer: every step's loss values,
     the returned (train_loss, lr), the final parameters;
 (c) EarlyStopper's decisions for every monitor on three scripted curves;
 (d) the optimizer state dicts (torch layout) the loop of (b) ends with, for SGD and RMSprop.
"""
from __future__ import annotations

import json
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle import gen_golden as G  # noqa: E402
from tests import train_ref as T  # noqa: E402
from gen_golden_eval import placeholders  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g13_train.npz")


class Config(dict):
    """easydict's EasyDict, as far as the reference's configs use it: a dict with attribute access, nested."""

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = Config(v) if isinstance(v, dict) and not isinstance(v, Config) else v

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    __setattr__ = dict.__setitem__


def config(optimizer, scheduler, epochs, opt_kw, diff_lr):
    return Config(model_name="JSPSR", optimizer=optimizer, optimizer_kwargs=dict(opt_kw, diff_lr=diff_lr), scheduler=scheduler,
                  scheduler_kwargs=dict(T.SCHED_KW), epochs=epochs, verbose=False, loss=dict(T.LOSS), train_num_visual=0,
                  num_train_sample=sum(T.BATCH_SIZES), train_batch_size=T.BATCH_SIZES[0], input_data=dict(T.INPUT_DATA),
                  monitor_value=None)


def momentum_of(group):
    return group["betas"][0] if "betas" in group else group["momentum"]


def main():
    G.import_reference()
    sys.modules["easydict"] = types.ModuleType("easydict")
    sys.modules["easydict"].EasyDict = Config
    placeholders(["piq", "skimage", "skimage.metrics", "kornia", "kornia.filters", "richdem", "hide_warnings", "affine",
                  "natsort", "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.axes_grid1", "seaborn", "pandas",
                  "prettytable", "rasterio", "rasterio.features", "rioxarray", "rioxarray.merge", "geopandas", "mapply",
                  "torchinfo", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.utils", "cv2",
                  "tifffile", "PIL", "PIL.Image", "osgeo", "tensorboardX", "torch.utils.tensorboard"])
    sys.modules["kornia.filters"].spatial_gradient = T.spatial_gradient
    import utils.common_config as cc
    import train.train_utils as tu
    import losses.loss_functions as lf
    lf.spatial_gradient = T.spatial_gradient

    def batch_pair_cpu(batch, model_name=None, input_data=None, gpu=0):
        inputs = [batch["lr_dem"]] + [batch[k] for k in ("image", "mask", "canopy", "coord") if k in input_data]
        return inputs, batch["hr_dem"], batch["base"], batch["meta"]

    tu.get_batch_pair = batch_pair_cpu

    store = {"seed": np.int64(T.SEED), "inputs_checksum": np.float64(T.inputs_checksum())}
    # (a) schedules
    for sched in T.SCHEDULERS:
        for opt in T.OPTIMIZERS:
            for diff in (False, True):
                for epochs in T.SCHEDULE_EPOCHS:
                    p = config(opt, sched, epochs, T.OPT_KW, diff)
                    net = T.small_net()
                    o = cc.get_optimizer(p, net)
                    s = cc.get_scheduler(p, o)
                    rows = []
                    for _ in range(epochs):
                        rows.append([[g["lr"], momentum_of(g)] for g in o.param_groups])
                        o.step()
                        s.step()
                    store[T.schedule_key(sched, opt, diff, epochs)] = np.array(rows, dtype=np.float64)
    # (b) epochs and (d) checkpoints
    for opt in T.OPTIMIZERS:
        p = config(opt, T.EPOCH_SCHEDULER, T.EPOCH_EPOCHS, T.EPOCH_OPT_KW[opt], False)
        net = T.small_net()
        crit = cc.get_criterion(p.loss)
        o = cc.get_optimizer(p, net)
        s = cc.get_scheduler(p, o)
        steps = []
        inner = crit.forward

        def recording(pred, gt, inner=inner, steps=steps):
            out = inner(pred, gt)
            steps.append([out[k].item() for k in ("L1", "L2", "Grad", "Total")])
            return out

        crit.forward = recording
        results = []
        for e in range(T.EPOCHS_RUN):
            loss, lr = tu.train_one_epoch(0, p, T.batches(), net, crit, o, s, (e + 1, p.epochs))
            results.append([loss, lr])
        store[f"epoch_{opt}_steps"] = np.array(steps, dtype=np.float64)
        store[f"epoch_{opt}_result"] = np.array(results, dtype=np.float64)
        store[f"epoch_{opt}_params"] = np.concatenate([q.detach().numpy().reshape(-1) for q in net.parameters()])
        if opt in ("SGD", "RMSprop"):
            sd = o.state_dict()
            store[f"ck_{opt}_groups"] = np.array(json.dumps(sd["param_groups"]))
            store[f"ck_{opt}_scheduler"] = np.array(json.dumps({k: v for k, v in s.state_dict().items()
                                                                   if isinstance(v, (int, float))}))
            for idx, st in sd["state"].items():
                for k, v in st.items():
                    store[f"ck_{opt}_state_{idx}_{k}"] = np.asarray(v.detach().numpy() if torch.is_tensor(v) else v)
    # (c) EarlyStopper
    table = {}
    for monitor in T.MONITORS:
        for name in T.CURVES:
            table[f"{monitor}/{name}"] = T.decisions(tu.EarlyStopper(T.PATIENCE, T.MIN_DELTA, monitor), T.curve(name))
    store["early_stop"] = np.array(json.dumps(table))
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
