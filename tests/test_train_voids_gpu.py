"""GPU: training and validating on a ground truth with voids (K19) -- `DeviceScenes(hr_nodata=)`, `batch["valid"]`, the
masked criterion inside `train_one_epoch` and `evaluate` -- on JSPSR nf 8 (the smallest model the training tests build),
three 72 / 80-px scenes whose hr_dem has -32767 and NaN holes, 64-px crops."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jspsr_amd import data as D
from jspsr_amd import evaluate as EV
from jspsr_amd import losses as L
from jspsr_amd import optim as O
from jspsr_amd import train as TR
from jspsr_amd.ddp import GradReducer
from oracle import jspsr_ref as R
from tests import batches_ref as B

DEV = "cuda:0"
IC = {"lr_dem": 1, "image": 3, "mask": 15}
SHAPES = [(72, 72), (72, 72), (80, 80)]
LOSS = {"L1": 1.0, "L2": 1.0, "Grad": 0.1, "Berhu": 0.2}


@pytest.fixture(scope="module")
def scenes():
    raw = B.make_scenes(SHAPES, seed=41)
    rs = np.random.RandomState(42)
    for i, s in enumerate(raw):
        hr = s["hr_dem"].copy()
        h, w = hr.shape[:2]
        hr[5:30, w - 20:] = -32767.0                       # a lake that touches the border
        hr[40 + i:52, 10:33] = np.nan                      # a cloud
        hr[rs.rand(h, w) < 0.05] = -32767.0                # sensor dropouts
        hr[0, 0] = np.inf
        s["hr_dem"] = hr
    kinds = {k: [s[k] for s in raw] for k in ("lr_dem", "hr_dem", "image", "mask")}
    with pytest.raises((AssertionError, ValueError)):      # without the keyword the store refuses such a ground truth
        D.DeviceScenes(**kinds, device=DEV, **B.PARAMS)
    return D.DeviceScenes(**kinds, device=DEV, hr_nodata=-32767, **B.PARAMS)


def random_batches(scenes):
    return D.RandomCropBatches(scenes, 2, 64, rng=np.random.RandomState(6), sampler=[0, 1, 2, 2, 1, 0])


def build():
    from jspsr_amd.JSPSR import Model
    m = Model(dict(IC, COP30=1), num_feature=8)
    m.load_state_dict(R.make_state_dict(R.jspsr_param_shapes(IC, 8), seed=43))
    m = m.to(DEV).train()
    red = GradReducer(m.parameters())
    red.watch_streams(m.side_streams("cuda"))
    opt = O.FlatSGD(red, lr=1e-3, momentum=0.9, weight_decay=1e-6)
    return m, red, opt, O.ConstantLR(opt), L.get_criterion(LOSS)


def test_train_one_epoch_on_voids(scenes):
    batches = list(random_batches(scenes))
    assert len(batches) == 3
    for b in batches:
        v = b["valid"]
        assert v.dtype == torch.uint8 and v.shape == b["hr_dem"].shape and 0 < int(v.sum()) < v.numel()
        assert torch.isfinite(b["hr_dem"][v != 0]).all() and not torch.isfinite(b["hr_dem"]).all()      # the voids are IN the target
    # by hand: the first step's gradients
    m, red, opt, sch, crit = build()
    inputs, gt, _, _ = D.batch_pair(batches[0], "JSPSR", IC)
    red.zero_grad()
    out = crit(m(*inputs), gt, valid=batches[0]["valid"])
    out["Total"].backward()
    red.finish()
    torch.cuda.synchronize()
    by_hand = red.flat.clone()
    assert torch.isfinite(by_hand).all() and by_hand.any()
    hand_values = {k: v.item() for k, v in out.items()}
    # the unmasked criterion on the same batch is what the feature is for: it is not finite
    assert not np.isfinite(crit(m(*inputs).detach(), gt)["Total"].item())
    # one step through train_one_epoch: the same gradients, bit for bit
    m, red, opt, sch, crit = build()
    start = [p.detach().clone() for p in m.parameters()]
    loss, lr, terms, _ = TR.train_one_epoch(m, batches[:1], crit, opt, sch, red, "JSPSR", IC)
    assert torch.equal(red.flat, by_hand)
    assert loss == hand_values["Total"] and terms == {k: hand_values[k] for k in LOSS}
    # and a whole epoch: finite losses, finite parameters, every parameter moved
    loss, lr, terms, ranges = TR.train_one_epoch(m, random_batches(scenes), crit, opt, sch, red, "JSPSR", IC, monitor_value=("grad",))
    assert np.isfinite(loss) and list(terms) == list(LOSS) and all(np.isfinite(v) for v in terms.values())
    assert np.all(ranges["grad"][:, 2] == 0)                                        # no non-finite gradient element in any step
    for p, q in zip(m.parameters(), start):
        assert torch.isfinite(p).all() and not torch.equal(p, q)


def test_graphed_step_refuses_batches_with_a_plane(scenes):
    from jspsr_amd.graph import GraphedStep
    m, red, opt, sch, crit = build()
    batches = list(random_batches(scenes))
    inputs, gt, _, _ = D.batch_pair(batches[0], "JSPSR", IC)
    clean = torch.where(batches[0]["valid"] != 0, gt, torch.full_like(gt, 0.5))       # the capture itself runs the unmasked step
    step = GraphedStep(m, red, opt, crit, inputs, clean, warmup=1)
    before = [p.detach().clone() for p in m.parameters()]
    with pytest.raises(NotImplementedError, match="GraphedStep"):
        TR.train_one_epoch(m, batches[1:], crit, opt, sch, red, "JSPSR", IC, step=step)
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), before))


def test_evaluate_on_voids(scenes):
    m, red, opt, sch, crit = build()
    m.eval()
    tiles = D.TileCropBatches(scenes, 3, 64, 4)
    scores, total, terms = EV.evaluate(m, tiles, crit, None, "JSPSR", IC)
    assert scores is None and np.isfinite(total) and list(terms) == list(LOSS) and all(np.isfinite(v) for v in terms.values())
    rows = []
    with torch.no_grad():
        for batch in tiles:
            inputs, gt, _, _ = D.batch_pair(batch, "JSPSR", IC)
            pred = m(*inputs)
            for i in range(gt.size(0)):
                out = crit(pred[i:i + 1], gt[i:i + 1], valid=batch["valid"][i:i + 1])
                rows.append({k: float(v.item()) for k, v in out.items()})
    assert len(rows) == 12
    for k in list(LOSS) + ["Total"]:
        want = sum(r[k] for r in rows) / len(rows)
        got = total if k == "Total" else terms[k]
        assert got == pytest.approx(want, rel=1e-12), k
    # a masked batch value is not the mean of its samples' values: the per-sample route is what the issue asks for
    meter = EV.PerformanceMeter({"RMSE": {"package": "local"}}, -80.0, 933.0, border=0.0, elev_log=True)
    with pytest.raises(NotImplementedError, match="meter"):
        EV.evaluate(m, tiles, crit, meter, "JSPSR", IC)
    with pytest.raises(ValueError, match="compare_input"):
        EV.evaluate(m, tiles, crit, None, "JSPSR", IC, compare_input=True)
