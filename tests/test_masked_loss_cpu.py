"""Masked losses and the validity plane of the store (K19) without a GPU: the fp64 restatement tests/masked_loss_ref.py
against the unmasked restatements it must reduce to with an all-ones plane (oracle.jspsr_ref.multi_loss,
tests/loss_menu_ref.py), `DeviceScenes(hr_nodata=, valid=)` on the host, header, binding and library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from oracle import jspsr_ref as R
from tests import loss_menu_ref as M
from tests import masked_loss_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(elev_min=-80, elev_max=933, elev_log=True)
ENTRIES = {"jspsr_loss_valid_workspace_bytes": 3, "jspsr_loss_valid_forward": 12, "jspsr_loss_valid_backward": 13,
           "jspsr_loss_menu_valid_workspace_bytes": 4, "jspsr_loss_menu_valid_forward": 14,
           "jspsr_loss_menu_valid_backward": 12, "jspsr_batch_valid": 9}


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 5, 3), (2, 1, 37, 53), (3, 2, 19, 70)])
def test_all_ones_plane_is_the_unmasked_restatement(shape):
    p, g = (torch.from_numpy(a).double() for a in V.pair(19, shape))
    ones = torch.ones(shape, dtype=torch.bool)
    x = p.clone().requires_grad_()
    got = V.multi_loss(x, g, ones)
    got["Total"].backward()
    y = p.clone().requires_grad_()
    want = R.multi_loss(y, g, 1.0, 1.0, 0.1)
    want["Total"].backward()
    for k in ("L1", "L2", "Grad", "Total"):
        assert rel(got[k].item(), want[k].item()) <= 1e-12, k
    assert (x.grad - y.grad).abs().max().item() <= 1e-12 * y.grad.abs().max().item()
    for name in ("l1", "l2", "bce", "berhu", "norm"):
        if name == "norm" and shape[1] != 1:
            continue
        v, gr = V.values_and_grad({name: 1.0}, p, g, ones)
        v64, g64 = M.value_and_grad(M.TERMS[name], p, g)
        assert rel(v[name], v64) <= 1e-12 and rel(v["Total"], v64) <= 1e-12, name
        assert (gr - g64).abs().max().item() <= 1e-12 * g64.abs().max().item(), name
    # a (B,1,H,W) plane is expanded over C
    v1, _ = V.values_and_grad({"L1": 1, "Grad": 0.1}, p, g, np.ones((shape[0], 1) + shape[2:], bool))
    v2, _ = V.values_and_grad({"L1": 1, "Grad": 0.1}, p, g, ones)
    assert v1 == v2


def test_restatement_counts_compacts_and_ignores_what_is_masked():
    p, g = (torch.from_numpy(a).double() for a in V.pair(20, (2, 1, 9, 11)))
    v = torch.ones(p.shape, dtype=torch.bool)
    v[0, 0, 0, 0] = False                                    # a corner void un-counts four outputs (the clamp)
    c = V.counted(v)
    assert int((~c).sum()) == 4 and not c[0, 0, :2, :2].any()
    v[1, 0, 4, 5] = False                                    # an interior void un-counts nine
    assert int((~V.counted(v)).sum()) == 13
    d = (p - g)
    vals, grad = V.values_and_grad({"L1": 1, "L2": 1, "Grad": 0.1}, p, g, v)
    assert rel(vals["L1"], d[v].abs().mean().item()) <= 1e-15 and rel(vals["L2"], (d[v] ** 2).mean().item()) <= 1e-15
    assert (grad[~v] == 0).all() and torch.isfinite(grad).all()
    for junk in (float("nan"), float("inf"), -32767.0):
        p2, g2 = p.clone(), g.clone()
        p2[~v], g2[~v] = junk, -junk
        vals2, grad2 = V.values_and_grad({"L1": 1, "L2": 1, "Grad": 0.1}, p2, g2, v)
        assert vals2 == vals and torch.equal(grad2, grad)
    none = torch.zeros(p.shape, dtype=torch.bool)
    vals0, grad0 = V.values_and_grad({"L1": 1, "L2": 1, "Grad": 0.1, "Berhu": 1, "BCE": 1, "Norm": 1}, p, g, none)
    assert all(x == 0.0 for x in vals0.values()) and not grad0.any()
    with pytest.raises(NotImplementedError):
        V.term("ssim", p, g, v)


# ---- the store ---------------------------------------------------------------------------------------------------------
def rasters(seed=4):
    rs = np.random.RandomState(seed)
    hrs = [rs.uniform(150, 400, s).astype(np.float32)[..., None] for s in ((7, 9), (6, 5))]
    lrs = [h + rs.uniform(-3, 3, h.shape).astype(np.float32) for h in hrs]
    return lrs, hrs, rs


def test_store_valid_plane():
    lrs, hrs, rs = rasters()
    plain = D.DeviceScenes(lrs, hrs, relative=True, device="cpu", **P)
    assert "valid" not in plain.store and plain.hr_nodata is None
    holes = [h.copy() for h in hrs]
    holes[0][1, 2], holes[0][6, 8], holes[0][3, 3] = -32767.0, np.nan, np.inf
    holes[1][0, 0] = -32767.0
    S = D.DeviceScenes(lrs, holes, relative=True, device="cpu", hr_nodata=-32767, **P)
    plane = S.store["valid"]
    assert plane.dtype == torch.uint8 and plane.numel() == 96 and plane.numel() % 4 == 0        # 63 + 30 pixels, padded
    want = np.concatenate([~D.void_pixels(h[..., 0], -32767).reshape(-1) for h in holes])
    assert np.array_equal(plane.numpy()[:93], want.astype(np.uint8)) and not plane.numpy()[93:].any()
    assert int(want.sum()) == 93 - 4
    assert S.store["hr_dem"].numpy().tobytes() == np.concatenate([h.reshape(-1) for h in holes]).tobytes()   # uploaded unchanged
    for k in ("lr_dem",):
        assert torch.equal(S.store[k], plain.store[k])
    assert S.base == plain.base and torch.equal(S.scene_table, plain.scene_table)
    # hr_nodata = NaN: not finite only
    N = D.DeviceScenes(lrs, [np.where(np.isfinite(h), h, np.nan).astype(np.float32) for h in holes], relative=True, device="cpu",
                       hr_nodata=float("nan"), elev_min=-40000, elev_max=933)
    assert int(N.store["valid"].sum()) == 93 - 2
    # the user's planes are ANDed in (bool, uint8 with any non-zero byte, a torch tensor)
    user = [rs.rand(7, 9) < 0.6, torch.from_numpy((rs.rand(6, 5) < 0.6).astype(np.uint8) * 9)]
    both = D.DeviceScenes(lrs, holes, relative=True, device="cpu", hr_nodata=-32767, valid=user, **P)
    want2 = want & np.concatenate([user[0].reshape(-1), user[1].numpy().reshape(-1) != 0])
    assert np.array_equal(both.store["valid"].numpy()[:93], want2.astype(np.uint8))
    only = D.DeviceScenes(lrs, hrs, relative=True, device="cpu", valid=user, **P)
    assert np.array_equal(only.store["valid"].numpy()[:93] != 0, np.concatenate([user[0].reshape(-1), user[1].numpy().reshape(-1) != 0]))
    ones = D.DeviceScenes(lrs, hrs, relative=True, device="cpu", hr_nodata=-32767, **P)
    assert ones.store["valid"].numpy()[:93].all()


def test_store_range_checks_and_refusals():
    lrs, hrs, rs = rasters()
    holes = [h.copy() for h in hrs]
    holes[0][1, 2], holes[1][2, 2] = -32767.0, np.nan
    with pytest.raises((AssertionError, ValueError)):                 # today's store refuses such rasters
        D.DeviceScenes(lrs, holes, relative=True, device="cpu", **P)
    D.DeviceScenes(lrs, holes, relative=True, device="cpu", hr_nodata=-32767, **P)       # the checks read valid pixels only
    high = [h.copy() for h in holes]
    high[1][4, 4] = 5000.0                                            # a VALID pixel out of range is still refused
    with pytest.raises(AssertionError, match="scene 1 hr_dem"):
        D.DeviceScenes(lrs, high, relative=True, device="cpu", hr_nodata=-32767, **P)
    mask = [np.ones((7, 9), bool), np.ones((6, 5), bool)]
    mask[1][4, 4] = False                                             # ... unless the user's plane takes it out
    D.DeviceScenes(lrs, high, relative=True, device="cpu", hr_nodata=-32767, valid=mask, **P)
    gone = [holes[0], np.full_like(holes[1], -32767.0)]
    gone[1][1, 1] = np.nan
    with pytest.raises(ValueError, match="scene second.*no valid pixel"):
        D.DeviceScenes(lrs, gone, relative=True, device="cpu", hr_nodata=-32767, ids=["first", "second"], **P)
    with pytest.raises(ValueError, match="scene first.*no valid pixel"):
        D.DeviceScenes(lrs, hrs, relative=True, device="cpu", valid=[np.zeros((7, 9), bool), mask[1]], ids=["first", "second"], **P)
    with pytest.raises(NotImplementedError, match="hr_dem.*hr_nodata"):
        D.DeviceScenes(lrs, hrs, relative=True, device="cpu", nodata=-32767, **P)
    bad_lr = [l.copy() for l in lrs]
    bad_lr[0][0, 0] = np.nan
    with pytest.raises(ValueError, match="lr_dem"):
        D.DeviceScenes(bad_lr, holes, relative=True, device="cpu", hr_nodata=-32767, **P)
    for bad in ([mask[0]], [mask[0], np.ones((6, 4), bool)], [mask[0], np.ones((6, 5), np.float32)]):
        with pytest.raises(ValueError, match="valid"):
            D.DeviceScenes(lrs, hrs, relative=True, device="cpu", valid=bad, **P)


# ---- header, binding, library ------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    assert _lib.ABI_VERSION == 25
    hdr = open(os.path.join(ROOT, "include", "jspsr_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for entry, n_args in ENTRIES.items():
        assert entry in _lib.SIGNATURES and hasattr(lib, entry), entry
        proto = re.search(r"\b(?:int|size_t)\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n_args, entry
    assert _lib.load().jspsr_abi_version() == 25
    for entry, n in (("jspsr_loss_forward", 11), ("jspsr_loss_backward", 12), ("jspsr_loss_menu_forward", 13),
                     ("jspsr_loss_menu_backward", 11), ("jspsr_batch_make", 16)):          # the unmasked entries are untouched
        proto = re.search(r"\bint\s+" + entry + r"\s*\((.*?)\);", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[entry][1]) == n, entry


def test_entries_refuse_bad_arguments_before_any_launch():
    """JSPSR_EINVAL before a launch (safe without a GPU: no device pointer is dereferenced)."""
    lib = _lib.load()
    x = ctypes.c_void_p(4096)
    labels = (b"loss_valid_forward", b"loss_valid_backward", b"loss_menu_valid_sum", b"loss_menu_valid_backward", b"batch_valid")
    before = {n: lib.jspsr_launch_count(n) for n in labels}
    slots, w, sw = (ctypes.c_int * 1)(3), (ctypes.c_double * 1)(1.0), (ctypes.c_double * 7)(*[1.0] * 7)
    assert lib.jspsr_loss_valid_forward(x, x, None, 1.0, 1.0, 0.1, x, x, 1, 8, 8, None) == -1
    assert b"loss_valid_forward" in lib.jspsr_last_error()
    assert lib.jspsr_loss_valid_forward(x, x, x, 1.0, 1.0, 0.1, x, x, 0, 8, 8, None) == -1
    assert lib.jspsr_loss_valid_backward(x, x, None, None, 1.0, 1.0, 0.1, x, x, 1, 8, 8, None) == -1
    assert lib.jspsr_loss_valid_workspace_bytes(0, 8, 8) == 0
    assert lib.jspsr_loss_valid_workspace_bytes(2, 8, 8) >= lib.jspsr_loss_workspace_bytes(2, 8, 8) + 16
    # SSIM (term bit 8) over a plane is not built
    assert lib.jspsr_loss_menu_valid_workspace_bytes(8, 1, 32, 32) == 0 and lib.jspsr_loss_menu_valid_workspace_bytes(9, 1, 32, 32) == 0
    assert lib.jspsr_loss_menu_valid_workspace_bytes(7, 1, 32, 32) > 0
    assert lib.jspsr_loss_menu_valid_forward(x, x, x, 9, 1, 32, 32, 1, slots, w, None, x, x, None) == -1
    assert b"SSIM" in lib.jspsr_last_error()
    assert lib.jspsr_loss_menu_valid_backward(x, x, x, 8, 1, 32, 32, sw, None, x, x, None) == -1
    assert lib.jspsr_loss_menu_valid_forward(x, x, None, 1, 1, 32, 32, 1, slots, w, None, x, x, None) == -1
    assert lib.jspsr_loss_menu_valid_forward(x, x, x, 2, 1, 32, 32, 1, slots, w, None, x, x, None) == -1      # slot 3 not in terms
    assert lib.jspsr_batch_valid(None, 64, x, x, 1, x, 1, 8, None) == -1 and b"batch_valid" in lib.jspsr_last_error()
    assert lib.jspsr_batch_valid(x, 0, x, x, 1, x, 1, 8, None) == -1
    assert lib.jspsr_batch_valid(x, 64, x, x, 1, x, 0, 8, None) == -1
    assert lib.jspsr_batch_valid(ctypes.c_void_p(4097), 64, x, x, 1, x, 1, 8, None) == -2
    assert before == {n: lib.jspsr_launch_count(n) for n in labels}
