"""K11 and the training loop on the MI355X: the flat optimizers against torch.optim, their two scalar forms and their
checkpoints, the fused gradient range, `optim.tensor_ranges`, and `train.train_one_epoch` / `train.fit` against the
reference-made fixture (tests/golden/g13_train.npz) and against hand-written loops over the same pieces.

Bounds.  Flat optimizer vs torch.optim on identical gradients, per tensor: max|flat - torch_fp32| <= 4 x max|torch_fp32 -
torch_fp64| + 1e-7, the fp32-vs-fp64 distance measured here on the CPU; the factor 4 is for a different but equally valid
operation order (fused multiply-add, a reciprocal for a division).  At 3 steps the project's bound rtol 1e-5, atol 1e-7
holds as well.  Per-step losses of an epoch against the reference's: the loss menu's 2e-6 x max(1, |ref|), widened per
step by the fp32-vs-fp64 difference of the same step's loss in a CPU torch rerun of the loop (what the drift of the
parameters does to that loss).  Everything else is compared bit for bit."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import evaluate as EV
from jspsr_amd import losses as L
from jspsr_amd import optim as O
from jspsr_amd import train as TR
from jspsr_amd.ddp import GradReducer
from tests import train_ref as T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_train.npz")
DEV = "cuda:0"
FLAT = {"SGD": O.FlatSGD, "Adam": O.FlatAdam, "AdamW": O.FlatAdamW, "RMSprop": O.FlatRMSprop}
TORCH = {"SGD": torch.optim.SGD, "Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW, "RMSprop": torch.optim.RMSprop}
STATE = {"SGD": ("momentum_buffer",), "Adam": ("exp_avg", "exp_avg_sq"), "AdamW": ("exp_avg", "exp_avg_sq"),
         "RMSprop": ("square_avg", "momentum_buffer")}


@pytest.fixture(scope="module")
def g13():
    z = dict(np.load(GOLDEN))
    assert float(z["inputs_checksum"]) == T.inputs_checksum()       # fail, never skip, if the inputs do not regenerate
    return z


class Three(torch.nn.Module):
    """Three tensors of sizes that exercise head, body and tail of the kernels; `c` is the second lr group."""

    def __init__(self, seed=0, dtype=torch.float32):
        super().__init__()
        rs = np.random.RandomState(seed)
        self.a = torch.nn.Parameter(torch.from_numpy(rs.standard_normal((3, 1000))).to(dtype))
        self.b = torch.nn.Parameter(torch.from_numpy(rs.standard_normal(1000)).to(dtype))
        self.c = torch.nn.Parameter(torch.from_numpy(rs.standard_normal(7)).to(dtype))


def grads(step, seed=11):
    rs = np.random.RandomState(seed + step)
    return [torch.from_numpy(rs.standard_normal(s) * 0.1).float() for s in ((3, 1000), (1000,), (7,))]


def kwargs(name, wd, momentum):
    kw = {"lr": 1e-2 if name == "SGD" else 1e-3, "weight_decay": wd}
    if name in ("SGD", "RMSprop"):
        kw["momentum"] = momentum
    return kw


def scheduler(name, opt):
    return O.get_scheduler({"scheduler": name, "epochs": 10, "scheduler_kwargs": {"warmup_epoch": 2, "max_lr": 5e-3, "step_size": 3,
                                                                                  "gamma": 0.5}}, opt)


def torch_run(name, sched, wd, momentum, steps, dtype):
    net = Three(dtype=dtype)
    opt = TORCH[name]([{"params": [net.a, net.b]}, {"params": [net.c], "lr": 3e-4}], **kwargs(name, wd, momentum))
    sch = scheduler(sched, opt)
    for i in range(steps):
        for p, g in zip(net.parameters(), grads(i)):
            p.grad = g.to(dtype)
        opt.step()
        if i % 2 == 1:
            sch.step()
    return [p.detach().clone() for p in net.parameters()]


def flat_run(name, sched, wd, momentum, steps, device_hyper=False, grad_range=False):
    net = Three().to(DEV)
    red = GradReducer(net.parameters())
    opt = FLAT[name](red, lr_overrides={net.c: 3e-4}, **kwargs(name, wd, momentum))
    if device_hyper:
        opt.enable_device_hyper()
    if grad_range:
        opt.fused_grad_range()
    sch = scheduler(sched, opt)
    for i in range(steps):
        opt.zero_grad()
        for p, g in zip(net.parameters(), grads(i)):
            p.grad.copy_(g)
        red.finish()
        opt.step()
        if i % 2 == 1:
            sch.step()
    return net, red, opt


@pytest.mark.parametrize("wd,momentum", [(1e-6, 0.0), (1e-2, 0.9)])
@pytest.mark.parametrize("sched", T.SCHEDULERS)
@pytest.mark.parametrize("name", T.OPTIMIZERS)
def test_flat_optimizer_matches_torch(name, sched, wd, momentum):
    for steps in (3, 20):
        t32 = torch_run(name, sched, wd, momentum, steps, torch.float32)
        t64 = torch_run(name, sched, wd, momentum, steps, torch.float64)
        net, _, _ = flat_run(name, sched, wd, momentum, steps)
        for k, (p, a, b) in enumerate(zip(net.parameters(), t32, t64)):
            ref_err = (a.double() - b).abs().max().item()
            err = (p.detach().cpu() - a).abs().max().item()
            print(f"{name} {sched} wd={wd} m={momentum} steps={steps} tensor {k}: |flat-torch32| {err:.3e}  |torch32-torch64| {ref_err:.3e}")
            assert err <= 4 * ref_err + 1e-7, (name, sched, steps, k, err, ref_err)
            if steps == 3:
                assert torch.allclose(p.detach().cpu(), a, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", T.OPTIMIZERS)
def test_argument_form_and_device_form_give_the_same_bits(name):
    for momentum in (0.0, 0.9):
        a, _, oa = flat_run(name, "CosineAnnealingLR", 1e-2, momentum, 7)
        b, _, ob = flat_run(name, "CosineAnnealingLR", 1e-2, momentum, 7, device_hyper=True)
        c, _, oc = flat_run(name, "CosineAnnealingLR", 1e-2, momentum, 7, device_hyper=True, grad_range=True)
        for other, oo in ((b, ob), (c, oc)):
            for p, q in zip(a.parameters(), other.parameters()):
                assert torch.equal(p, q), name
            for key in STATE[name]:
                x, y = getattr(oa, key), getattr(oo, key)
                assert (x is None and y is None) or torch.equal(x, y), (name, key)


@pytest.mark.parametrize("layout", ["flat", "torch"])
@pytest.mark.parametrize("name", ["SGD", "Adam", "RMSprop"])
def test_flat_optimizer_checkpoint_round_trip_is_bit_exact(name, layout, tmp_path):
    """3 steps -> torch.save / torch.load -> a fresh optimizer -> 3 more steps equal 6 uninterrupted steps bit for bit."""
    a, _, oa = flat_run(name, "StepLR", 1e-2, 0.9, 6)
    b, _, ob = flat_run(name, "StepLR", 1e-2, 0.9, 3)
    path = tmp_path / "ck.pt"
    torch.save({"optimizer": ob.state_dict(layout=layout), "state_dict": b.state_dict()}, path)
    ck = torch.load(path)
    c = Three(seed=5).to(DEV)
    rc = GradReducer(c.parameters())
    oc = FLAT[name](rc, lr_overrides={c.c: 3e-4}, **kwargs(name, 1e-2, 0.9))
    sc = scheduler("StepLR", oc)
    c.load_state_dict(ck["state_dict"])
    oc.load_state_dict(ck["optimizer"])
    sc.load_state_dict({"last_epoch": 1})
    for i in range(3, 6):
        oc.zero_grad()
        for p, g in zip(c.parameters(), grads(i)):
            p.grad.copy_(g)
        rc.finish()
        oc.step()
        if i % 2 == 1:
            sc.step()
    for p, q in zip(a.parameters(), c.parameters()):
        assert torch.equal(p, q)
    for key in STATE[name]:
        assert torch.equal(getattr(oa, key), getattr(oc, key)), key


@pytest.mark.parametrize("name", ["SGD", "Adam", "RMSprop"])
def test_flat_optimizer_exchanges_checkpoints_with_torch(name):
    """Mirrors test_flat_adamw_exchanges_checkpoints_with_torch_adamw: a torch-written state resumes here, a state written
    here (layout="torch") resumes in torch; three more steps on either side agree with the uninterrupted torch run."""
    kw = kwargs(name, 1e-6, 0.9)

    def torch_opt(net):
        return TORCH[name]([{"params": [net.a, net.b]}, {"params": [net.c], "lr": 3e-4}], **kw)

    def tsteps(net, opt, lo, hi):
        for i in range(lo, hi):
            for p, g in zip(net.parameters(), grads(i)):
                p.grad = g.to(p.device)
            opt.step()

    def fsteps(net, red, opt, lo, hi):
        for i in range(lo, hi):
            opt.zero_grad()
            for p, g in zip(net.parameters(), grads(i)):
                p.grad.copy_(g)
            red.finish()
            opt.step()

    ref = Three().to(DEV)
    ropt = torch_opt(ref)
    tsteps(ref, ropt, 0, 3)
    mid_model, mid_opt = {k: v.clone() for k, v in ref.state_dict().items()}, copy.deepcopy(ropt.state_dict())
    tsteps(ref, ropt, 3, 6)
    # torch checkpoint -> flat
    a = Three(seed=9).to(DEV)
    a.load_state_dict(mid_model)
    ra = GradReducer(a.parameters())
    oa = FLAT[name](ra, lr_overrides={a.c: 3e-4}, **kw)
    oa.load_state_dict(mid_opt)
    fsteps(a, ra, oa, 3, 6)
    for pa, pr in zip(a.parameters(), ref.parameters()):
        assert torch.allclose(pa, pr, rtol=1e-5, atol=1e-7)
    # flat checkpoint (torch layout) -> torch
    b = Three().to(DEV)
    rb = GradReducer(b.parameters())
    ob = FLAT[name](rb, lr_overrides={b.c: 3e-4}, **kw)
    fsteps(b, rb, ob, 0, 3)
    c = Three(seed=9).to(DEV)
    c.load_state_dict(b.state_dict())
    copt = torch_opt(c)
    copt.load_state_dict(ob.state_dict(layout="torch"))
    tsteps(c, copt, 3, 6)
    for pc, pr in zip(c.parameters(), ref.parameters()):
        assert torch.allclose(pc, pr, rtol=1e-5, atol=1e-7)
    with pytest.raises(ValueError, match="unknown optimizer checkpoint format|not an optimizer state dict"):
        oa.load_state_dict({"state": {}, "param_groups": [{"lr": 1e-3}]})
    with pytest.raises(ValueError, match="groups its parameters differently"):
        oa.load_state_dict(TORCH[name](Three().parameters(), lr=1e-3).state_dict())


@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_reference_made_checkpoint_loads(g13, name):
    """Fixture (d): the optimizer state dict the reference's loop ended with (torch layout) scatters into the flat buffers."""
    groups = json.loads(str(g13[f"ck_{name}_groups"]))
    net = T.small_net().to(DEV)
    params = list(net.parameters())
    state = {}
    for idx in range(len(params)):
        st = {}
        for key in STATE[name] + ("step",):
            arr = g13.get(f"ck_{name}_state_{idx}_{key}")
            if arr is not None:
                st[key] = torch.from_numpy(np.asarray(arr))
        state[idx] = st
    red = GradReducer(net.parameters())
    opt = FLAT[name](red, lr=1.0, momentum=0.5, weight_decay=0.0)
    opt.load_state_dict({"state": state, "param_groups": groups})
    assert opt.lr == groups[0]["lr"] and opt.momentum == 0.9 and opt.weight_decay == 1e-6
    if name == "RMSprop":
        assert opt.steps == T.EPOCHS_RUN * len(T.BATCH_SIZES) and opt.alpha == 0.99
    for idx, p in enumerate(params):
        off, n = opt._slices[id(p)]
        for key in STATE[name]:
            want = torch.from_numpy(g13[f"ck_{name}_state_{idx}_{key}"]).reshape(-1)
            assert torch.equal(getattr(opt, key)[off:off + n].cpu(), want), (idx, key)


# ---- the fused gradient range -------------------------------------------------------------------------------------------
def raw_step(kind, p, g, s1, s2, rng, ws, lr=1e-3):
    lib = _lib.load()
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.jspsr_optim_step(kind, ptr(p), ptr(g), ptr(s1), ptr(s2), p.numel(), lr, 0.9, 0.999 if kind in (1, 2) else 0.99,
                                    1e-8, 1e-2, 1, None, ptr(rng), ptr(ws), torch.cuda.current_stream().cuda_stream), "jspsr_optim_step")


def fresh_range():
    return torch.tensor([999.0, -999.0, 0.0, 0.0], device=DEV)


def workspace():
    return torch.empty(_lib.load().jspsr_optim_workspace_bytes() // 4, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("n", [1, 3, 5, 4096 + 3, 10 ** 6 + 1])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_fused_gradient_range_equals_min_max(kind, n):
    ws = workspace()
    gen = torch.Generator(device=DEV).manual_seed(n + kind)
    for mis in (0, 1, 3):                                  # equally misaligned starts
        base = [torch.randn(n + 4, device=DEV, generator=gen) for _ in range(4)]
        base[2].abs_(), base[3].abs_()
        with_range = [t.clone()[mis:mis + n] for t in base]
        without = [t.clone()[mis:mis + n] for t in base]
        states = lambda v: (v[2], v[3]) if kind in (1, 2, 3) else (v[2], None)
        rng = fresh_range()
        raw_step(kind, with_range[0], with_range[1], *states(with_range), rng, ws)
        raw_step(kind, without[0], without[1], *states(without), None, None)
        g = with_range[1]
        assert rng.tolist() == [g.min().item(), g.max().item(), 0.0, 0.0], (kind, n, mis)
        for a, b in zip(with_range, without):              # the parameters and the state do not depend on the range pointer
            assert torch.equal(a, b), (kind, n, mis)
        assert not torch.equal(with_range[0], base[0][mis:mis + n])


def test_fused_gradient_range_combines_and_keeps_the_reference_start_values():
    ws = workspace()
    n = 5000
    mk = lambda: [torch.randn(n, device=DEV) for _ in range(2)] + [torch.rand(n, device=DEV) for _ in range(2)]
    # two ranges fold into the same four floats
    a, b = mk(), mk()
    rng = fresh_range()
    raw_step(2, a[0], a[1], a[2], a[3], rng, ws)
    raw_step(2, b[0], b[1], b[2], b[3], rng, ws)
    both = torch.cat((a[1], b[1]))
    assert rng.tolist() == [both.min().item(), both.max().item(), 0.0, 0.0]
    # all above 999: min stays 999; all below -999: max stays -999
    hi, lo = mk(), mk()
    hi[1].abs_().add_(1000.0)
    lo[1].abs_().neg_().sub_(1000.0)
    rng = fresh_range()
    raw_step(0, hi[0], hi[1], hi[2], None, rng, ws)
    assert rng.tolist() == [999.0, hi[1].max().item(), 0.0, 0.0]
    rng = fresh_range()
    raw_step(0, lo[0], lo[1], lo[2], None, rng, ws)
    assert rng.tolist() == [lo[1].min().item(), -999.0, 0.0, 0.0]
    # 2 NaN and 1 inf: counted, and the range is that of the rest
    c = mk()
    c[1][7], c[1][4000], c[1][123] = float("nan"), float("nan"), float("inf")
    finite = c[1][torch.isfinite(c[1])]
    rng = fresh_range()
    raw_step(3, c[0], c[1], c[2], c[3], rng, ws)
    assert rng.tolist() == [finite.min().item(), finite.max().item(), 3.0, 0.0]
    # no finite gradient at all: the reference's start values come back, [999, -999]
    d = mk()
    d[1].fill_(float("nan"))
    rng = fresh_range()
    raw_step(1, d[0], d[1], d[2], d[3], rng, ws)
    assert rng.tolist() == [999.0, -999.0, float(n), 0.0]


def test_optimizer_grad_range_attribute_covers_every_group():
    for name in T.OPTIMIZERS:
        net, red, opt = flat_run(name, "ConstantLR", 1e-6, 0.9, 2, grad_range=True)
        assert len(opt.param_groups) == 2
        assert opt.grad_range.tolist() == [red.flat.min().item(), red.flat.max().item(), 0.0, 0.0], name
        plain, _, _ = flat_run(name, "ConstantLR", 1e-6, 0.9, 2)
        for p, q in zip(net.parameters(), plain.parameters()):
            assert torch.equal(p, q), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tensor_ranges_equal_torch(dtype):
    gen = torch.Generator(device=DEV).manual_seed(3)
    sizes = [(1,), (7, 3), (2, 1, 64, 64), (4097,), (3, 5, 17), (100001,), (8, 1, 128, 128), (2,)]
    tensors = [(torch.randn(s, device=DEV, generator=gen) * (k + 1)).to(dtype) for k, s in enumerate(sizes)]
    for count in range(1, 9):
        table = O.tensor_ranges(tensors[:count])
        assert tuple(table.shape) == (count, 4)
        want = [[t.min().float().item(), t.max().float().item(), 0.0, 0.0] for t in tensors[:count]]
        assert table.tolist() == want, count
    mixed = [tensors[2].float(), tensors[3].to(torch.bfloat16)]
    mixed[0][0, 0, 3, 3] = float("nan")
    table = O.tensor_ranges(mixed)
    fin = mixed[0][torch.isfinite(mixed[0])]
    assert table[0].tolist() == [fin.min().item(), fin.max().item(), 1.0, 0.0]
    assert table[1].tolist() == [mixed[1].min().float().item(), mixed[1].max().float().item(), 0.0, 0.0]
    with pytest.raises(ValueError):
        O.tensor_ranges(tensors + tensors[:1])
    with pytest.raises(ValueError):
        O.tensor_ranges([tensors[0].double()])


# ---- train_one_epoch ------------------------------------------------------------------------------------------------
def device_batches():
    return [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()} for b in T.batches()]


def epoch_config(name):
    return {"model_name": "JSPSR", "optimizer": name, "optimizer_kwargs": dict(T.EPOCH_OPT_KW[name], diff_lr=False),
            "scheduler": T.EPOCH_SCHEDULER, "scheduler_kwargs": dict(T.SCHED_KW), "epochs": T.EPOCH_EPOCHS}


def torch_multi_loss(pred, gt):
    l1, l2 = (pred - gt).abs().mean(), ((pred - gt) ** 2).mean()
    lg = (T.spatial_gradient(pred) - T.spatial_gradient(gt)).abs().mean()
    return T.LOSS["L1"] * l1 + T.LOSS["L2"] * l2 + T.LOSS["Grad"] * lg


def cpu_losses(name, dtype):
    """The loop of fixture (b) as plain torch on the CPU in `dtype`: the Total loss of every step."""
    net = T.small_net().to(dtype)
    p = epoch_config(name)
    kw = {k: v for k, v in T.EPOCH_OPT_KW[name].items() if k != "momentum" or name in ("SGD", "RMSprop")}
    opt = TORCH[name](net.parameters(), **kw)
    sch = O.get_scheduler(p, opt)
    out = []
    for _ in range(T.EPOCHS_RUN):
        for b in T.batches():
            opt.zero_grad()
            loss = torch_multi_loss(net(b["lr_dem"].to(dtype), b["image"].to(dtype)), b["hr_dem"].to(dtype))
            loss.backward()
            opt.step()
            out.append(loss.item())
        sch.step()
    return np.array(out)


@pytest.mark.parametrize("name", T.OPTIMIZERS)
def test_train_one_epoch_matches_the_reference_epochs(g13, name, monkeypatch):
    want_steps, want_result = g13[f"epoch_{name}_steps"], g13[f"epoch_{name}_result"]
    drift = np.abs(cpu_losses(name, torch.float32) - cpu_losses(name, torch.float64))
    net = T.small_net().to(DEV)
    red = GradReducer(net.parameters())
    p = epoch_config(name)
    opt = O.get_optimizer(p, net, red)
    sch = O.get_scheduler(p, opt)
    crit = L.get_criterion(T.LOSS)
    batches = device_batches()
    syncs = []

    def counted(fn, what):
        def wrapper(*a, **k):
            syncs.append(what)
            return fn(*a, **k)
        return wrapper

    n = len(T.BATCH_SIZES)
    for e in range(T.EPOCHS_RUN):
        seen = {}
        inner = crit.forward

        def recording(pred, gt, inner=inner, seen=seen):
            out = inner(pred, gt)
            seen.setdefault("rows", []).append(torch.stack([out[k].detach() for k in ("L1", "L2", "Grad", "Total")]))
            return out

        crit.forward = recording
        with monkeypatch.context() as mp:
            mp.setattr(torch.Tensor, "cpu", counted(torch.Tensor.cpu, "cpu"))
            mp.setattr(torch.Tensor, "item", counted(torch.Tensor.item, "item"))
            mp.setattr(torch.Tensor, "tolist", counted(torch.Tensor.tolist, "tolist"))
            mp.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize, "synchronize"))
            del syncs[:]
            loss, lr, terms, ranges = TR.train_one_epoch(net, batches, crit, opt, sch, red, "JSPSR", T.INPUT_DATA,
                                                         monitor_value=("grad", "input", "pred"))
            assert syncs == ["cpu"], syncs                      # exactly one host synchronisation per epoch
        crit.forward = inner
        rows = torch.stack(seen["rows"]).cpu().numpy().astype(np.float64)
        want = want_steps[e * n:(e + 1) * n]
        for i in range(n):
            tol = 2e-6 * np.maximum(1.0, np.abs(want[i])) + drift[e * n + i]
            print(f"{name} epoch {e} step {i}: |loss - reference| {np.abs(rows[i] - want[i]).max():.3e}  drift {drift[e * n + i]:.3e}")
            assert np.all(np.abs(rows[i] - want[i]) <= tol), (name, e, i, rows[i], want[i], drift[e * n + i])
        assert lr == want_result[e, 1]
        mon = TR.LossMonitor(["L1", "L2", "Grad", "Total"])
        mon.update_rows(rows.astype(np.float32), T.BATCH_SIZES)
        assert loss == mon.avg["Total"] and terms == {k: mon.avg[k] for k in ("L1", "L2", "Grad")}
        assert abs(loss - want_result[e, 0]) <= 2e-6 * max(1.0, abs(want_result[e, 0])) + drift[e * n:(e + 1) * n].max()
        assert set(ranges) == {"grad", "input", "gt", "pred"} and all(v.shape == (n, 3) for v in ranges.values())
        assert ranges["input"][-1].tolist() == [batches[-1]["lr_dem"].min().item(), batches[-1]["lr_dem"].max().item(), 0.0]
        assert ranges["gt"][0].tolist() == [batches[0]["hr_dem"].min().item(), batches[0]["hr_dem"].max().item(), 0.0]
        assert ranges["grad"][-1].tolist() == [red.flat.min().item(), red.flat.max().item(), 0.0]
        assert opt.grad_range is None


def test_train_one_epoch_jspsr_equals_the_hand_written_loop():
    """JSPSR nf 8, image + mask, 64 x 64 crops, 3 steps via DeviceScenes / RandomCropBatches and get_criterion: the loss
    sequence equals that of the hand-written loop over the same pieces bit for bit -- with the monitors on and off, and
    with the step replayed from a hipGraph."""
    from jspsr_amd import data as D
    from jspsr_amd.JSPSR import Model
    from jspsr_amd.graph import GraphedStep
    from oracle import jspsr_ref as R
    from tests import batches_ref as B
    ic = {"lr_dem": 1, "image": 3, "mask": 15}
    sd = R.make_state_dict(R.jspsr_param_shapes(ic, 8), seed=31)
    raw = B.make_scenes([(150, 150), (140, 140), (130, 160)], seed=29)
    scenes = D.DeviceScenes(**{k: [s[k] for s in raw] for k in ("lr_dem", "hr_dem", "image", "mask")}, device=DEV, **B.PARAMS)
    order = [0, 1, 2, 2, 1, 0]

    def batches():
        return D.RandomCropBatches(scenes, 2, 64, rng=np.random.RandomState(5), sampler=order)

    def build():
        m = Model(dict(ic, COP30=1), num_feature=8)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        red = GradReducer(m.parameters())
        red.watch_streams(m.side_streams("cuda"))
        opt = O.FlatSGD(red, lr=1e-3, momentum=0.9, weight_decay=1e-6)
        return m, red, opt, O.ConstantLR(opt), L.get_criterion({"L1": 1.0, "L2": 1.0, "Grad": 0.1})

    m, red, opt, sch, crit = build()
    by_hand = []
    for batch in batches():
        crit.reset()
        inputs, gt, _, _ = D.batch_pair(batch, "JSPSR", ic)
        red.zero_grad()
        out = crit(m(*inputs), gt)
        out["Total"].backward()
        red.finish()
        opt.step()
        by_hand.append(out["Total"].item())
    assert len(by_hand) == 3
    final = [p.detach().clone() for p in m.parameters()]

    def losses_of(monitor_value):
        m, red, opt, sch, crit = build()
        seen = []
        inner = crit.forward
        crit.forward = lambda pred, gt: (lambda out: (seen.append(out["Total"].detach()), out)[1])(inner(pred, gt))
        loss, lr, terms, ranges = TR.train_one_epoch(m, batches(), crit, opt, sch, red, "JSPSR", ic, monitor_value=monitor_value)
        for p, q in zip(m.parameters(), final):
            assert torch.equal(p, q)
        mon = TR.LossMonitor(["Total"])
        mon.update_rows(np.array([[v] for v in by_hand], dtype=np.float32), [2, 2, 2])
        assert loss == mon.avg["Total"] and lr == 1e-3 and list(terms) == ["L1", "L2", "Grad"]
        return [v.item() for v in seen], ranges

    off, ranges = losses_of(())
    assert off == by_hand and ranges == {}
    on, ranges = losses_of(("grad", "input", "pred"))
    assert on == by_hand and set(ranges) == {"grad", "input", "gt", "pred"}
    assert np.all(ranges["grad"][:, 0] < 0) and np.all(ranges["grad"][:, 1] > 0) and np.all(ranges["grad"][:, 2] == 0)

    # the step replayed from a graph: 1 eager warm-up step inside the constructor on the first batch, then replays
    m, red, opt, sch, crit = build()
    opt.fused_grad_range()                     # before the capture, so the captured step writes the range
    it = iter(batches())
    first = next(it)
    inputs, gt, _, _ = D.batch_pair(first, "JSPSR", ic)
    step = GraphedStep(m, red, opt, crit, inputs, gt, warmup=1)
    rest = list(it)
    loss, lr, terms, ranges = TR.train_one_epoch(m, rest, crit, opt, sch, red, "JSPSR", ic, monitor_value=("grad",), step=step)
    mon = TR.LossMonitor(["Total"])
    mon.update_rows(np.array([[v] for v in by_hand[1:]], dtype=np.float32), [2, 2])
    assert loss == mon.avg["Total"] and terms == {}
    for p, q in zip(m.parameters(), final):
        assert torch.equal(p, q)
    assert ranges["grad"].shape == (2, 3) and ranges["grad"][-1].tolist() == [red.flat.min().item(), red.flat.max().item(), 0.0]
    opt.grad_range = None                      # asked for a range the captured step does not write: a clear error
    with pytest.raises(RuntimeError, match="before the capture"):
        TR.train_one_epoch(m, rest, crit, opt, sch, red, "JSPSR", ic, monitor_value=("grad",), step=step)


# ---- fit ---------------------------------------------------------------------------------------------------------------
METRICS = {"RMSE": {"package": "local"}, "PSNR": {"package": "local"}}


def new_meter():
    return EV.PerformanceMeter(METRICS, -80.0, 929.0, border=0.0, elev_log=True)


def fit_config(epochs, **kw):
    return dict({"model_name": "JSPSR", "input_data": T.INPUT_DATA, "epochs": epochs, "optimizer": "SGD",
                 "optimizer_kwargs": {"lr": 1e-2, "momentum": 0.9, "weight_decay": 1e-6, "diff_lr": False},
                 "scheduler": "CosineAnnealingLR", "scheduler_kwargs": {"warmup_epoch": 0}, "val_interval": 2, "val_start_epoch": 1,
                 "best_metric": "RMSE", "early_stop": {"patience": 3, "monitor": "val_loss"}, "monitor_value": None}, **kw)


def test_fit_small_model_history_and_best_checkpoint(tmp_path):
    p = fit_config(8)
    net = T.small_net().to(DEV)
    red = GradReducer(net.parameters())
    opt = O.get_optimizer(p, net, red)
    sch = O.get_scheduler(p, opt)
    batches = device_batches()
    path = tmp_path / "best.pt"
    hist = TR.fit(p, net, batches[:4], batches[4:], L.get_criterion(T.LOSS), opt, sch, red, new_meter(), checkpoint_path=path)
    assert len(hist) == 9 and hist[0]["epoch"] == 0 and set(hist[0]["scores"]) == set(METRICS) and "input_scores" in hist[0]
    for e, h in enumerate(hist[1:]):
        assert h["epoch"] == e + 1 and h["evaluated"] == EV.do_eval(8, e, 0, 0, 2, 1), e
    assert [h["epoch"] for h in hist[1:] if h["evaluated"]] == [1, 2, 4, 5, 6, 7, 8]
    # the best checkpoint is the epoch validate_results picks, replayed here from the recorded scores
    best, best_epoch = hist[0]["scores"], None
    for h in hist[1:]:
        if h["evaluated"]:
            better, best = EV.validate_results(h["scores"], best, "RMSE")
            assert better == h["is_better"] and best == h["best"]
            if better:
                best_epoch = h["epoch"]
    assert best_epoch is not None
    ck = torch.load(path)
    assert ck["epoch"] == best_epoch and ck["best_result"] == best
    assert set(ck) == {"optimizer", "state_dict", "scheduler", "epoch", "best_result"}
    assert hist[2]["lr"] < hist[1]["lr"] == 1e-2


class Toy(torch.nn.Module):
    """Element-wise on purpose: its gradients are bit-reproducible, so any difference after a resume is the loop's."""

    def __init__(self):
        super().__init__()
        rs = np.random.RandomState(77)
        self.a = torch.nn.Parameter(torch.from_numpy(1 + 0.1 * rs.standard_normal((1, 1, T.SIDE, T.SIDE))).float())
        self.b = torch.nn.Parameter(torch.from_numpy(0.1 * rs.standard_normal((1, 3, T.SIDE, T.SIDE))).float())
        self.c = torch.nn.Parameter(torch.from_numpy(0.01 * rs.standard_normal((1, 1, T.SIDE, T.SIDE))).float())

    def forward(self, lr_dem, image):
        return lr_dem * self.a + torch.tanh(image * self.b)[:, 0:1] + self.c


@pytest.mark.parametrize("name", ["SGD", "Adam"])
def test_fit_resume_equals_the_uninterrupted_run(name, tmp_path):
    p = fit_config(6, optimizer=name, val_interval=1, resume=True,
                   optimizer_kwargs={"lr": 1e-2 if name == "SGD" else 1e-3, "momentum": 0.9, "weight_decay": 1e-6, "diff_lr": False})
    batches = device_batches()

    def run(resume_from=None, checkpoint=None):
        net = Toy().to(DEV)
        red = GradReducer(net.parameters())
        opt = O.get_optimizer(p, net, red)
        sch = O.get_scheduler(p, opt)
        hist = TR.fit(p, net, batches[:4], batches[4:], L.get_criterion(T.LOSS), opt, sch, red, new_meter(),
                      checkpoint_path=checkpoint, resume_from=resume_from)
        return net, opt, hist

    a, oa, ha = run(checkpoint=str(tmp_path / "ck_{epoch}.pt"))
    improved = [h["epoch"] for h in ha[1:] if h.get("is_better")]
    assert 4 in improved, improved                          # the toy improves every epoch
    b, ob, hb = run(resume_from=tmp_path / "ck_4.pt")
    assert [h["epoch"] for h in hb] == [4, 5, 6]
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    for key in STATE[name]:
        assert torch.equal(getattr(oa, key), getattr(ob, key)), key
    assert [h["train_loss"] for h in hb[1:]] == [h["train_loss"] for h in ha[5:]]
