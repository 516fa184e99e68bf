"""CPU: the loss menu's fp64 restatements (tests/loss_menu_ref.py) against the reference-made fixture
tests/golden/g10_loss_menu.npz, piq's SSIM restatement against itself and the reference's local ssim, and the host logic
of jspsr_amd.losses.get_loss / get_criterion (building a criterion launches nothing)."""
import os

import numpy as np
import pytest
import torch

from tests import loss_menu_ref as M

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_loss_menu.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


def test_fixture_inputs_regenerate_bit_for_bit(z):
    pred, gt = M.inputs(int(z["seed"]), tuple(z["shape"]))
    assert np.array_equal(pred, z["pred"]) and np.array_equal(gt, z["gt"]), "seeded inputs changed: regenerate g10"
    assert M.checksum([pred, gt]) == float(z["input_checksum"])
    for i in range(len(M.SSIM_SHAPES)):
        assert M.checksum(M.ssim_inputs(i)) == float(z[f"ssim_local_{i}_checksum"]), i


@pytest.mark.parametrize("name", ["l1", "l2", "mse", "bce", "vanilla", "berhu", "norm"])
def test_restatement_equals_reference(z, name):
    v, g = M.value_and_grad(M.TERMS[name], z["pred"], z["gt"])
    ref_v, ref_g = float(z[f"{name}_value"]), torch.from_numpy(z[f"{name}_grad"])
    assert abs(v - ref_v) <= 1e-12 * abs(ref_v), (v, ref_v)
    scale = ref_g.abs().max().item()
    if name == "norm":      # the reference's autograd leaves ~2e-16 residues where |p| > eps: absolute floor there
        assert (g - ref_g).abs().max().item() <= 1e-12 * scale + 1e-12
        ana = M.norm_grad(torch.from_numpy(z["pred"]).double(), torch.from_numpy(z["gt"]).double())
        assert (ana - ref_g).abs().max().item() <= 1e-12 * scale + 1e-12
        assert (ana != 0).sum().item() == 4      # the four exact zeros of pred take the |p| <= eps branch
    else:
        assert (g - ref_g).abs().max().item() <= 1e-12 * scale


def test_berhu_degenerate_departure(z):
    """pred == gt: loss 0 like the reference; our gradient is 0 where the reference's is NaN (documented departure)."""
    assert float(z["berhu_equal_value"]) == 0.0 and bool(z["berhu_equal_grad_nan"])
    v, g = M.value_and_grad(M.berhu, z["gt"], z["gt"])
    assert v == 0.0 and torch.count_nonzero(g).item() == 0


def test_local_window_is_the_reference_window(z):
    from jspsr_amd.metrics import local_window
    w = local_window()
    assert torch.equal(w, torch.from_numpy(z["local_window"]))
    assert w.argmax().item() == 0 and not torch.allclose(w, w.flip(0))   # asymmetric, decaying: not a Gaussian


def test_local_ssim_restatement_matches_reference(z):
    """The SSIM formula of the piq restatement, run with the reference's window and zero padding, reproduces the
    reference's own local ssim: in fp32 (as the reference computes it) to the last bits, in fp64 within 1e-6 beyond the
    fp32 rounding the reference itself carries (its E[x^2] - mu^2 cancels in fp32)."""
    w32 = torch.from_numpy(z["local_window"])
    for i in range(len(M.SSIM_SHAPES)):
        ref = float(z[f"ssim_local_{i}"])
        p, g = (torch.from_numpy(a) for a in M.ssim_inputs(i))
        v32 = M.ssim_local(g, p, w32).item()
        v = M.ssim_local(g.double(), p.double(), w32.double()).item()
        assert abs(v32 - ref) <= 1e-7, (i, v32, ref)
        assert abs(v - ref) <= 1e-6 + abs(v32 - v), (i, v, ref)
        assert abs(M.ssim_map(g.double(), p.double(), w32.double(), 5, separable=True).mean().item() - v) <= 1e-12


def test_piq_restatement_self_consistent():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 19, 23, generator=g, dtype=torch.float64)
    y = (x + 0.1 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    a, b = M.ssim_piq(x, y, separable=True).item(), M.ssim_piq(x, y, separable=False).item()
    assert abs(a - b) <= 1e-13, (a, b)
    assert abs(M.ssim_piq(x, x).item() - 1.0) <= 1e-13
    assert M.ssim_map(x, y, M.gauss1d(), 0).shape == (2, 3, 9, 13)       # valid map: (H-10) x (W-10)
    w = M.gauss1d()
    assert abs(w.sum().item() - 1) < 1e-15 and torch.allclose(w, w.flip(0), rtol=0, atol=1e-17)
    xg = (0.05 + 0.9 * torch.rand(1, 1, 12, 13, generator=g, dtype=torch.float64)).requires_grad_()
    yg = torch.rand(1, 1, 12, 13, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda t: M.ssim_loss(t, yg), (xg,), eps=1e-6, atol=1e-7)


def test_multi_and_single_reference_bookkeeping(z):
    """The reference MultiLoss (non-unit weights) and SingleLoss from the fixture equal the restated weighted sums."""
    keys = [str(k) for k in z["multi_keys"]]
    assert keys == ["L1", "Berhu", "BCE", "Norm", "mse", "Total"]
    ws = z["multi_weights"]
    p, g = torch.from_numpy(z["pred"]).double().requires_grad_(), torch.from_numpy(z["gt"]).double()
    vals = [M.TERMS[k.lower()](p, g) for k in keys[:-1]]
    total = sum(w * v for w, v in zip(ws, vals))
    total.backward()
    ref = z["multi_values"]
    for v, r in zip([v.item() for v in vals] + [total.item()], ref):
        assert abs(v - r) <= 1e-12 * abs(r), (v, r)
    assert (p.grad - torch.from_numpy(z["multi_grad"])).abs().max().item() <= 1e-12 * np.abs(z["multi_grad"]).max() + 1e-12
    assert [str(k) for k in z["single_keys"]] == ["Berhu", "Total"]
    assert z["single_values"][0] == z["single_values"][1] == z["berhu_value"]
    assert np.array_equal(z["single_grad"], z["berhu_grad"])


def test_get_loss_names_and_errors():
    from jspsr_amd.losses import LossTerm, get_loss
    for name in ("l1", "L1", "l2", "MSE", "mse", "vanilla", "BCE", "edge", "Grad", "berhu", "BerHu", "norm", "SSIM"):
        assert isinstance(get_loss(name), LossTerm)
    for bad in ("charbonnier", "tv", "l3", ""):
        with pytest.raises(NotImplementedError, match=f"Undefined loss: {bad}$"):
            get_loss(bad)


def test_get_criterion_host_logic():
    from jspsr_amd.losses import Criterion, get_criterion
    c = get_criterion({"L1": 1, "L2": 1, "Grad": 0.1})
    assert isinstance(c, Criterion) and not c.single
    assert c.spec.keys == ["L1", "L2", "Grad"] and c.spec.terms == 0 and c.spec.base_w == (1.0, 1.0, 0.1)
    c = get_criterion({"Berhu": 0.2, "L1": 1, "SSIM": 0.5, "mse": 2, "l2": 3})
    assert c.spec.keys == ["Berhu", "L1", "SSIM", "mse", "l2"]          # user's spelling, config order
    assert c.spec.weights == [0.2, 1.0, 0.5, 2.0, 3.0]
    assert c.spec.slots == [3, 0, 6, 1, 1] and c.spec.terms == 1 | 8
    assert c.spec.slot_w == [1.0, 5.0, 0.0, 0.2, 0.0, 0.0, 0.5] and c.spec.base
    s = get_criterion({"SSIM": 0.5})                                     # one key: weight 1, whatever is configured
    assert s.single and s.spec.weights == [1.0] and s.spec.terms == 8 and not s.spec.base
    assert str(s).startswith("SingleLoss:: SSIM") and str(c).startswith("MultiLoss:: ['Berhu', 'L1'")
    s.out = {"x": 1}
    s.reset()
    assert s.out == {}
    with pytest.raises(NotImplementedError, match="Undefined loss: Charbonnier"):
        get_criterion({"L1": 1, "Charbonnier": 1})
    with pytest.raises(ValueError):
        get_criterion({})


def test_criterion_shape_rules_raise_before_launch():
    """Norm needs C = 1, SSIM H, W >= 11 (ValueError); CPU tensors are refused (no fallback) -- all before a launch."""
    from jspsr_amd.losses import get_criterion
    spec = get_criterion({"Norm": 1, "L1": 1}).spec
    x = torch.zeros(1, 2, 16, 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        spec.check(x, x)
