"""K9 on the MI355X: jspsr_batch_make through jspsr_amd.data, against the reference-made fixture
(tests/golden/g11_batches.npz) and the numpy restatement (tests/batches_ref.py)."""
import os

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import data as D
from jspsr_amd import tiles as T
from tests import batches_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_batches.npz")
DEV = "cuda:0"
DEM_TOL = 2e-7           # numpy's fp32 log vs the device logf: one ulp, divided by log(1013)
KINDS = ("lr_dem", "hr_dem", "image", "mask", "canopy", "coord")


def device_scenes(scenes, **kw):
    p = dict(R.PARAMS, **kw)
    kinds = {k: [s[k] for s in scenes] for k in ("lr_dem", "hr_dem", "image", "mask", "canopy") if k in scenes[0]}
    return D.DeviceScenes(**kinds, device=DEV, **p)


def check(got: dict, ref: dict, where):
    for kind, v in ref.items():
        g = got[kind]
        if "dem" in kind:
            err = np.abs(g.astype(np.float64) - v.astype(np.float64)).max()
            assert err <= DEM_TOL, (where, kind, err)
        else:
            assert np.array_equal(g, v), (where, kind, np.argwhere(g != v)[:4])


def launches():
    return _lib.load().jspsr_launch_count(b"batch_make")


@pytest.fixture(scope="module")
def g11():
    z = np.load(GOLDEN)
    scenes = R.make_scenes()
    assert str(z["scenes_checksum"]) == R.scenes_checksum(scenes), "synthetic scenes differ from the ones the fixture was made on"
    return z, scenes


def test_fixture_random_pass(g11):
    z, scenes = g11
    S = device_scenes(scenes)
    it = D.RandomCropBatches(S, 4, R.K, rng=np.random.RandomState(R.DRAW_SEED), sampler=R.ORDER, drop_last=False)
    j = 0
    for batch in it:
        for b, m in enumerate(batch["meta"]):
            got = {k: batch[k][b].cpu().numpy() for k in ("lr_dem", "hr_dem", "image", "mask", "canopy")}
            check(got, {k: z[f"r{j}_{k}"] for k in got}, j)
            a = m["augmentation"]
            assert tuple(m["bbox"]) == tuple(z[f"r{j}_bbox"]) and [a["rot90"], a["flip_lr"], a["flip_ud"]] == list(z[f"r{j}_aug"])
            assert np.float32(m["base"]) == z[f"r{j}_base"] == batch["base"][b].item()
            j += 1
    assert j == len(R.ORDER)


def test_fixture_tile_pass(g11):
    z, scenes = g11
    S = device_scenes([scenes[i] for i in R.TILE_SCENES])
    j = 0
    for batch in D.TileCropBatches(S, 5, R.K, R.TILE_N):
        for b, m in enumerate(batch["meta"]):
            got = {k: batch[k][b].cpu().numpy() for k in ("lr_dem", "hr_dem", "image", "mask", "canopy")}
            check(got, {k: z[f"t{j}_{k}"] for k in got}, j)
            assert tuple(m["bbox"]) == tuple(z[f"t{j}_bbox"])
            j += 1
    assert j == len(R.TILE_SCENES) * R.TILE_N


ODD = [(141, 139), (203, 171), (77, 95), (131, 133)]


@pytest.mark.parametrize("k", [37, 128, 130])
def test_all_d4_codes_odd_scenes_and_patch_sizes(k):
    """Every (angle, lr, ud) on scenes of odd, unequal sizes, local coordinates included; k not a tile multiple too."""
    scenes = R.make_scenes(ODD, seed=31)
    S = device_scenes(scenes, coord="local", relative=(k != 128), elev_log=(k != 130), elev_min=-80, elev_max=933)
    p = dict(R.PARAMS, relative=(k != 128), elev_log=(k != 130))
    fits = [i for i, (h, w) in enumerate(ODD) if h >= k and w >= k]
    rs = np.random.RandomState(k)
    rows, refs = [], []
    for code in range(16):
        s = fits[code % len(fits)]
        h, w = ODD[s]
        y0, x0 = int(rs.randint(0, h - k + 1)), int(rs.randint(0, w - k + 1))
        base = np.min(scenes[s]["lr_dem"]) if p["relative"] else 0
        rows.append([s, y0, x0, code, np.float32(base).view(np.int32), 0, 0, 0])
        full = dict(scenes[s], coord=R.local_coord(h, w))
        crop = {kk: R.gather(a, y0, x0, k, code) for kk, a in full.items()}
        refs.append(R.to_tensor(crop, p, base))
    table = torch.tensor(rows, dtype=torch.int32, device=DEV)
    outs = {kk: (torch.full((16, S.channels[kk], k, k), -7.0, device=DEV), 0) for kk in S.kinds}
    n0 = launches()
    S.make(table, k, outs)
    torch.cuda.synchronize()
    assert launches() == n0 + 1
    for b in range(16):
        check({kk: outs[kk][0][b].cpu().numpy() for kk in S.kinds}, refs[b], (k, b))


def test_random_draws_against_the_restatement_at_the_config_patch():
    scenes = R.make_scenes([(334, 334), (301, 290), (140, 150)], seed=5, coord=False)
    S = device_scenes(scenes, coord="local")
    order = [2, 0, 1, 1, 0, 2]
    it = D.RandomCropBatches(S, 3, 128, rng=np.random.RandomState(9), sampler=order)
    ref = R.random_pass([dict(s, coord=R.local_coord(*s["lr_dem"].shape[:2])) for s in scenes], R.PARAMS, 128, order,
                        np.random.RandomState(9))
    j = 0
    for batch in it:
        for b in range(3):
            out, base, bbox, aug = ref[j]
            check({k: batch[k][b].cpu().numpy() for k in S.kinds}, out, j)
            m = batch["meta"][b]
            assert tuple(m["bbox"]) == bbox and tuple(m["augmentation"].values()) == aug
            j += 1
    assert j == len(order)


def test_one_launch_per_batch_and_concat_layout():
    scenes = R.make_scenes([(90, 90), (77, 83), (64, 70)], seed=8)
    S = device_scenes(scenes, coord="local")
    g = [torch.Generator().manual_seed(4) for _ in range(2)]
    split = D.RandomCropBatches(S, 2, 44, rng=np.random.RandomState(2), generator=g[0], drop_last=False)
    cat = D.RandomCropBatches(S, 2, 44, rng=np.random.RandomState(2), generator=g[1], drop_last=False, concat=True)
    n0 = launches()
    a = list(split)
    assert launches() == n0 + len(a) == n0 + 2
    c = list(cat)
    assert launches() == n0 + 4
    for x, y in zip(a, c):
        ref = torch.cat([x[k] for k in D.CONCAT_ORDER], dim=1)
        assert y["images"].shape == ref.shape and torch.equal(y["images"], ref)
        assert torch.equal(x["hr_dem"], y["hr_dem"]) and x["meta"] == y["meta"]
        inputs, gt, base, meta = D.batch_pair(y, "EDSR", {"lr_dem": 1, "image": 3, "mask": 15, "canopy": 1, "coord": 2})
        assert len(inputs) == 1 and inputs[0].data_ptr() == y["images"].data_ptr()     # the kernel's tensor, no copy
        inputs, gt, base, meta = D.batch_pair(x, "JSPSR", {"lr_dem": 1, "image": 3, "mask": 15})
        assert [t.data_ptr() for t in inputs] == [x["lr_dem"].data_ptr(), x["image"].data_ptr(), x["mask"].data_ptr()]
    with pytest.raises(ValueError):
        D.batch_pair(a[0], "EDSR", {"lr_dem": 1, "image": 3})


def test_back_to_back_batches_equal_synchronised_ones():
    """20 one-batch epochs issued with no host synchronisation -- 20 table uploads in flight -- equal the same 20 made
    with a synchronize() after each."""
    scenes = R.make_scenes([(150, 150), (133, 141)], seed=12)
    S = device_scenes(scenes)
    runs = []
    for sync in (False, True):
        it = D.RandomCropBatches(S, 2, 96, rng=np.random.RandomState(21), generator=torch.Generator().manual_seed(3))
        got = []
        for _ in range(20):
            for batch in it:
                got.append((batch["lr_dem"], batch["image"], batch["mask"], batch["canopy"], batch["hr_dem"], batch["base"]))
                if sync:
                    torch.cuda.synchronize()
        torch.cuda.synchronize()
        runs.append([tuple(t.cpu() for t in g) for g in got])
    assert len(runs[0]) == 20
    for x, y in zip(*runs):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    assert not all(torch.equal(runs[0][0][0], r[0]) for r in runs[0][1:])     # the batches do differ


def test_tile_batches_equal_crop_tiles():
    scenes = R.make_scenes([(70, 70), (96, 96)], seed=13)
    S = device_scenes(scenes, coord="local")
    k, n = 32, 9
    tiles = list(D.TileCropBatches(S, 9, k, n))
    assert len(tiles) == 2
    for s, (h, w) in enumerate([(70, 70), (96, 96)]):
        whole = {kk: (torch.empty((1, S.channels[kk], h, w), device=DEV), 0) for kk in S.kinds}
        row = [[s, 0, 0, 0, np.float32(S.base[s]).view(np.int32), 0, 0, 0]]
        S.make(torch.tensor(row, dtype=torch.int32, device=DEV), h, whole)
        for kk in S.kinds:
            assert torch.equal(tiles[s][kk], T.crop_tiles(whole[kk][0][0], k, n)), (s, kk)


def test_models_train_on_device_batches():
    from jspsr_amd.EDSR import EDSR
    from jspsr_amd.JSPSR import Model
    scenes = R.make_scenes([(80, 80), (72, 76)], seed=17)
    S = device_scenes(scenes)
    torch.manual_seed(0)
    ic = {"lr_dem": 1, "image": 3, "mask": 15}
    jspsr = Model(dict(ic, COP30=1), num_feature=8).to(DEV).train()
    for batch in D.RandomCropBatches(S, 2, 64, rng=np.random.RandomState(1)):
        inputs, gt, base, meta = D.batch_pair(batch, "JSPSR", ic)
        loss = ((jspsr(*inputs) - gt) ** 2).mean()
        loss.backward()
    g = [p.grad for p in jspsr.parameters() if p.grad is not None]
    assert g and all(torch.isfinite(t).all() for t in g) and torch.isfinite(loss)
    edsr = EDSR(in_channels=20, out_channels=1, n_resblocks=2, n_features=32, scale=1).to(DEV).train()
    for batch in D.RandomCropBatches(S, 2, 64, rng=np.random.RandomState(1), concat=True):
        inputs, gt, base, meta = D.batch_pair(batch, "EDSR", {"lr_dem": 1, "image": 3, "mask": 15, "canopy": 1})
        assert inputs[0].shape == (2, 20, 64, 64)
        loss = ((edsr(*inputs) - gt) ** 2).mean()
        loss.backward()
    g = [p.grad for p in edsr.parameters() if p.grad is not None]
    assert g and all(torch.isfinite(t).all() for t in g) and torch.isfinite(loss)
