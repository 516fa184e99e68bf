"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/g10_loss_menu.npz: the loss menu made by the reference's own code
(losses.loss_schemes get_loss / SingleLoss / MultiLoss, losses.loss_functions BerhuLoss / SurfaceNormalLoss,
evaluation.metrics gaussian / ssim), imported as oracle/gen_golden.py:gen_host_side does (placeholder modules for the
packages this image lacks: piq, kornia, skimage, richdem, hide_warnings, affine).  SSIMLoss and EdgeLoss need piq and
kornia and are NOT generated (tests/loss_menu_ref.py restates them; see its docstring).

Run where the reference tree is available (never on the GPU box):

    python tools/gen_golden_losses.py

Inputs come from numpy's legacy RandomState stream (tests/loss_menu_ref.py:dem_pair); the fixture stores the seed and
checksums, so the tests regenerate them and fail on a mismatch.
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402
from tests import loss_menu_ref as M  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g10_loss_menu.npz")
NAMES = ("l1", "l2", "mse", "bce", "vanilla", "berhu", "norm")


def main():
    G.import_reference()
    for name in ("piq", "skimage", "skimage.metrics", "kornia", "kornia.filters", "richdem", "hide_warnings", "affine"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].metrics = sys.modules["skimage.metrics"]
    sys.modules["kornia"].filters = sys.modules["kornia.filters"]
    sys.modules["kornia.filters"].spatial_gradient = None
    sys.modules["hide_warnings"].hide_warnings = lambda f=None, **k: (f if f is not None else (lambda g: g))
    sys.modules["affine"].Affine = None
    sys.modules["piq"].ssim = None
    import evaluation.metrics as em
    import losses.loss_schemes as ls

    pred, gt = M.inputs()
    store = {"seed": np.int64(M.SEED), "shape": np.array(M.SHAPE), "pred": pred, "gt": gt,
             "input_checksum": np.float64(M.checksum([pred, gt]))}
    p64, g64 = torch.from_numpy(pred).double(), torch.from_numpy(gt).double()
    for name in NAMES:
        p = p64.clone().requires_grad_()
        v = ls.get_loss(name)(p, g64)
        v.backward()
        store[f"{name}_value"] = np.float64(v.item())
        store[f"{name}_grad"] = p.grad.numpy()
        # the restatement must agree with the reference before anything is stored
        rv, rg = M.value_and_grad(M.TERMS[name], pred, gt)
        assert abs(rv - v.item()) <= 1e-12 * abs(v.item()), (name, rv, v.item())
        floor = 1e-12 if name != "norm" else 1e-9
        assert (rg - p.grad).abs().max().item() <= floor * max(1.0, p.grad.abs().max().item()), name
    # BerHu at pred == gt: loss 0; the reference's gradient is NaN there (stored to document the departure)
    p = g64.clone().requires_grad_()
    v = ls.get_loss("berhu")(p, g64)
    v.backward()
    store["berhu_equal_value"] = np.float64(v.item())
    store["berhu_equal_grad_nan"] = np.bool_(torch.isnan(p.grad).all().item())
    # the local ssim's window and two odd-shaped local ssim values (fp32, as the reference computes them)
    store["local_window"] = em.gaussian(11, 1.5).numpy()
    for i in range(len(M.SSIM_SHAPES)):
        sp, sg = M.ssim_inputs(i)
        store[f"ssim_local_{i}_checksum"] = np.float64(M.checksum([sp, sg]))
        store[f"ssim_local_{i}"] = np.float64(em.ssim(torch.from_numpy(sg), torch.from_numpy(sp), size_average=True).item())
    # a MultiLoss over torch-only terms with non-unit weights, and a SingleLoss built the way get_criterion builds one
    weights = {"L1": 0.7, "Berhu": 0.3, "BCE": 0.25, "Norm": 0.05, "mse": 2.0}
    crit = ls.MultiLoss(**{k: {"loss_fn": ls.get_loss(k), "weight": w} for k, w in weights.items()})
    p = p64.clone().requires_grad_()
    out = crit(p, g64)
    out["Total"].backward()
    store["multi_keys"] = np.array(list(out))
    store["multi_weights"] = np.array(list(weights.values()))
    store["multi_values"] = np.array([out[k].item() for k in out])
    store["multi_grad"] = p.grad.numpy()
    single = ls.SingleLoss(**{"Berhu": {"loss_fn": ls.get_loss("Berhu"), "weight": 1}})
    p = p64.clone().requires_grad_()
    out = single(p, g64)
    out["Total"].backward()
    store["single_keys"] = np.array(list(out))
    store["single_values"] = np.array([out[k].item() for k in out])
    store["single_grad"] = p.grad.numpy()
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
