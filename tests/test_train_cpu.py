"""The training loop without a GPU: `optim.get_scheduler` / `get_optimizer`, `train.EarlyStopper` and
`train.LossMonitor` against the numbers the reference's own code produced (tests/golden/g13_train.npz,
tools/gen_golden_train.py).

Bounds.  Schedules: |value - fixture| <= 1e-10 x the sequence's largest value, for the learning rates and for momentum /
beta1.  torch's cosine schedule is a recursion: 300 epochs x ~10 double operations x 1.1e-16 is about 3e-13 of the largest
term; 1e-10 leaves a few hundred times that and is still four orders below the 6e-8 at which an fp32 kernel argument
could tell two learning rates apart.  WarmupStepLR is compared with ==.  EarlyStopper's decisions and LossMonitor's
means are compared exactly."""
import json
import os

import numpy as np
import pytest
import torch

from jspsr_amd import optim as O
from jspsr_amd import train as TR
from jspsr_amd.ddp import GradReducer
from tests import train_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_train.npz")
SCHEDULE_CASES = [(s, o, d, e) for s in T.SCHEDULERS for o in T.OPTIMIZERS for d in (False, True) for e in T.SCHEDULE_EPOCHS]


@pytest.fixture(scope="module")
def g13():
    return dict(np.load(GOLDEN))


def config(optimizer, scheduler, epochs, opt_kw, diff_lr, model_name="JSPSR"):
    return {"model_name": model_name, "optimizer": optimizer, "optimizer_kwargs": dict(opt_kw, diff_lr=diff_lr),
            "scheduler": scheduler, "scheduler_kwargs": dict(T.SCHED_KW), "epochs": epochs}


class Groups:
    """A stand-in with torch-style param_groups, laid out as the reference's get_optimizer lays the named optimizer out."""

    def __init__(self, optimizer, diff_lr):
        extra = {"momentum": T.OPT_KW["momentum"]} if optimizer in ("SGD", "RMSprop") else {"betas": (0.9, 0.999)}
        self.param_groups = [dict(lr=T.OPT_KW["lr"], **extra)] + ([dict(lr=0.0003, **extra)] if diff_lr else [])


def momentum_of(g):
    return g["betas"][0] if "betas" in g else g["momentum"]


def test_fixture_inputs_regenerate(g13):
    assert int(g13["seed"]) == T.SEED
    assert float(g13["inputs_checksum"]) == T.inputs_checksum()


@pytest.mark.parametrize("scheduler,optimizer,diff_lr,epochs", SCHEDULE_CASES)
def test_schedule_matches_the_reference(g13, scheduler, optimizer, diff_lr, epochs):
    want = g13[T.schedule_key(scheduler, optimizer, diff_lr, epochs)]          # (epochs, groups, [lr, momentum])
    opt = Groups(optimizer, diff_lr)
    sch = O.get_scheduler(config(optimizer, scheduler, epochs, T.OPT_KW, diff_lr), opt)
    got = []
    for _ in range(epochs):
        got.append([[g["lr"], momentum_of(g)] for g in opt.param_groups])
        sch.step()
    got = np.array(got, dtype=np.float64)
    assert got.shape == want.shape
    if scheduler == "WarmupStepLR":
        assert np.array_equal(got, want)
    for col in (0, 1):
        err = np.abs(got[..., col] - want[..., col]).max()
        print(f"{scheduler} {optimizer} diff_lr={diff_lr} {epochs}: column {col} max err {err:.3e} of {want[..., col].max():.3e}")
        assert err <= 1e-10 * want[..., col].max()
    # a resume from {"last_epoch"} alone is exact
    opt2 = Groups(optimizer, diff_lr)
    sch2 = O.get_scheduler(config(optimizer, scheduler, epochs, T.OPT_KW, diff_lr), opt2)
    assert set(sch.state_dict()) == {"last_epoch"}
    sch2.load_state_dict({"last_epoch": 5})
    assert [[g["lr"], momentum_of(g)] for g in opt2.param_groups] == got[5].tolist()


def test_schedules_drive_the_flat_optimizers_groups():
    """On the real classes (CPU tensors: construction and param_groups only): OneCycleLR moves `momentum` of FlatSGD /
    FlatRMSprop and `betas[0]` of FlatAdam / FlatAdamW, 0.95 -> 0.85 -> 0.95, and overwrites every group's lr."""
    for name, key in (("sgd", "momentum"), ("rmsprop", "momentum"), ("adam", "betas"), ("adamw", "betas")):
        net = T.small_net()
        opt = O.get_optimizer(config(name, "OneCycleLR", 10, T.OPT_KW, True), net, GradReducer(net.parameters()))
        assert len(opt.param_groups) == 2 and opt.param_groups[1]["lr"] == 0.0003
        sch = O.get_scheduler({"scheduler": "onecyclelr", "epochs": 10, "scheduler_kwargs": {"max_lr": 1e-3}}, opt)
        seen = []
        for _ in range(10):
            g = opt.param_groups[1]
            seen.append(g[key][0] if key == "betas" else g[key])
            assert g["lr"] == opt.param_groups[0]["lr"]
            sch.step()
        assert seen[0] == 0.95 and abs(min(seen) - 0.85) < 1e-12 and abs(seen[-1] - 0.95) < 1e-12, (name, seen)
        if key == "betas":
            assert opt.param_groups[0]["betas"][1] == 0.999


def test_get_optimizer_maps_its_arguments():
    net = T.small_net()
    kw = {"lr": 2e-3, "momentum": 0.8, "weight_decay": 3e-5}
    for name, cls in (("SGD", O.FlatSGD), ("adam", O.FlatAdam), ("AdamW", O.FlatAdamW), ("RMSprop", O.FlatRMSprop)):
        opt = O.get_optimizer(config(name, "ConstantLR", 4, kw, False), net, GradReducer(net.parameters()))
        assert type(opt) is cls and opt.lr == 2e-3 and opt.weight_decay == 3e-5 and len(opt.param_groups) == 1
        if cls in (O.FlatSGD, O.FlatRMSprop):
            assert opt.momentum == 0.8 and opt.param_groups[0]["momentum"] == 0.8 and opt.momentum_buffer is not None
        else:
            assert opt.betas == (0.9, 0.999) and opt.eps == 1e-8
        if cls is O.FlatRMSprop:
            assert opt.alpha == 0.99 and opt.eps == 1e-8
        assert opt.grad_range is None
    opt = O.get_optimizer(config("adamw", "ConstantLR", 4, kw, True), net, GradReducer(net.parameters()))
    second = {id(p) for n, p in net.named_parameters() if "postprocessor" in n}
    assert [g["lr"] for g in opt.param_groups] == [2e-3, 0.0003]
    assert {i for i, g in opt._group_of.items() if g is opt.param_groups[1]} == second
    with pytest.raises(NotImplementedError, match="different learning rates"):
        O.get_optimizer(config("adamw", "ConstantLR", 4, kw, True, model_name="EDSR"), net, GradReducer(net.parameters()))
    with pytest.raises(NotImplementedError, match="Undefined optimizer: lion"):
        O.get_optimizer(config("lion", "ConstantLR", 4, kw, False), net, GradReducer(net.parameters()))


def test_get_scheduler_maps_its_arguments():
    opt = Groups("AdamW", False)
    s = O.get_scheduler({"scheduler": "WarmupStepLR", "epochs": 30, "scheduler_kwargs": {}}, opt)
    assert type(s) is O.WarmupStepLR and (s.warmup_epoch, s.step_size, s.gamma) == (0, 10, 0.1)      # not the constructor's
    s = O.get_scheduler({"scheduler": "warmupsteplr", "epochs": 30, "scheduler_kwargs": {"warmup_epoch": 2, "step_size": 7, "gamma": 0.5}}, opt)
    assert (s.warmup_epoch, s.step_size, s.gamma) == (2, 7, 0.5)
    s = O.get_scheduler({"scheduler": "StepLR", "epochs": 30, "scheduler_kwargs": {}}, opt)
    assert type(s) is O.StepLR and (s.step_size, s.gamma) == (10, 0.1)
    s = O.get_scheduler({"scheduler": "CosineAnnealingLR", "epochs": 30, "scheduler_kwargs": {}}, opt)
    assert type(s) is O.CosineAnnealingLR and (s.T_max, s.eta_min) == (30, 1e-6)
    s = O.get_scheduler({"scheduler": "OneCycleLR", "epochs": 30, "scheduler_kwargs": {}}, Groups("AdamW", False))
    assert type(s) is O.OneCycleLR and s.max_lr == 0.1 and s.total_steps == 30 and s.start_lr == 0.1 / 90
    assert type(O.get_scheduler({"scheduler": "constantlr", "epochs": 3, "scheduler_kwargs": {}}, opt)) is O.ConstantLR
    with pytest.raises(NotImplementedError, match="Undefined scheduler: poly"):
        O.get_scheduler({"scheduler": "poly", "epochs": 3, "scheduler_kwargs": {}}, opt)


def test_early_stopper_decisions_match_the_reference(g13):
    table = json.loads(str(g13["early_stop"]))
    assert set(table) == {f"{m}/{c}" for m in T.MONITORS for c in T.CURVES}
    for monitor in T.MONITORS:
        for name in T.CURVES:
            got = T.decisions(TR.EarlyStopper(T.PATIENCE, T.MIN_DELTA, monitor), T.curve(name))
            assert got == table[f"{monitor}/{name}"], (monitor, name)
    # the quirk: the score monitors decide as val_loss does
    for name in T.CURVES:
        assert table[f"val_rmse/{name}"] == table[f"val_loss/{name}"] == table[f"val_psnr/{name}"]
    # fixed=True compares the monitored score, higher-is-better for PSNR: on the curve whose loss wanders upwards while
    # the PSNR keeps improving it never stops, the reference's does
    fixed = T.decisions(TR.EarlyStopper(T.PATIENCE, T.MIN_DELTA, "val_psnr", fixed=True), T.curve("noisy"))
    assert fixed != table["val_psnr/noisy"] and not any(fixed) and any(table["val_psnr/noisy"])
    assert TR.EarlyStopper(None)(1.0) is False
    with pytest.raises(NotImplementedError):
        TR.EarlyStopper(3, monitor="val_psnr")(1.0, 1.0, {"RMSE": 1.0})


def test_loss_monitor_means_equal_the_reference_bit_for_bit(g13):
    for opt in T.OPTIMIZERS:
        steps, result = g13[f"epoch_{opt}_steps"], g13[f"epoch_{opt}_result"]
        n = len(T.BATCH_SIZES)
        assert steps.shape == (T.EPOCHS_RUN * n, 4)
        for e in range(T.EPOCHS_RUN):
            mon = TR.LossMonitor(["L1", "L2", "Grad", "Total"])
            # the values as a device table hands them over: fp32 numbers (the fixture holds the .item() of fp32 tensors)
            rows = steps[e * n:(e + 1) * n].astype(np.float32)
            assert np.array_equal(rows.astype(np.float64), steps[e * n:(e + 1) * n])
            mon.update_rows(rows, T.BATCH_SIZES)
            assert mon.avg["Total"] == result[e, 0], (opt, e)
            assert mon.count == sum(T.BATCH_SIZES)


def test_checkpoint_helpers_round_trip_on_cpu(tmp_path):
    """save_checkpoint writes main.py's five keys with the optimizer in torch's layout; load_state_dict copies only the
    entries whose key and size match; load_resume_state_dict honours `resume`."""
    net = T.small_net()
    red = GradReducer(net.parameters())
    opt = O.FlatSGD(red, lr=1e-2, momentum=0.9)
    sch = O.StepLR(opt, 2, 0.5)
    sch.step(), sch.step()
    path = tmp_path / "ck.pt"
    TR.save_checkpoint(path, net, opt, sch, 7, {"RMSE": 1.5})
    ck = torch.load(path)
    assert set(ck) == {"optimizer", "state_dict", "scheduler", "epoch", "best_result"}
    assert all("params" in g for g in ck["optimizer"]["param_groups"]) and ck["scheduler"] == {"last_epoch": 2}
    torch.optim.SGD(T.small_net().parameters(), lr=1.0, momentum=0.9).load_state_dict(ck["optimizer"])       # torch takes it
    other = T.small_net(seed=T.SEED + 50)
    red2 = GradReducer(other.parameters())
    opt2 = O.FlatSGD(red2, lr=1.0, momentum=0.9)
    sch2 = O.StepLR(opt2, 2, 0.5)
    model, start, best, o, s = TR.load_resume_state_dict(other, opt2, sch2, path, resume=True)
    assert start == 7 and best == {"RMSE": 1.5} and o is opt2 and s is sch2 and sch2.last_epoch == 2 and opt2.lr == 5e-3
    for a, b in zip(net.parameters(), other.parameters()):
        assert torch.equal(a, b)
    model, start, best, o, s = TR.load_resume_state_dict(T.small_net(), None, sch2, path, resume=False)
    assert start == 0 and s is None
    # a foreign entry and one of another size are left out
    tgt = T.small_net(seed=3)
    keep = tgt.conv1.weight.clone()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    sd["conv1.weight"] = torch.zeros(2, 2)
    sd["not.there"] = torch.zeros(1)
    TR.load_state_dict(tgt, sd)
    assert torch.equal(tgt.conv1.weight, keep) and torch.equal(tgt.conv2.weight, net.conv2.weight)
