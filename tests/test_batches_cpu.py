"""K9 host side: the draws, the sampler, the D4 map and the argument checks of jspsr_batch_make, against
tests/golden/g11_batches.npz (made by the reference's own transforms, tools/gen_golden_batches.py) and numpy."""
import ctypes
import os

import numpy as np
import pytest
import torch

from jspsr_amd import data as D
from tests import batches_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_batches.npz")


@pytest.fixture(scope="module")
def g11():
    z = np.load(GOLDEN)
    scenes = R.make_scenes()
    # the fixture's inputs are regenerated here: a different stream is a failure, never a skip
    assert str(z["scenes_checksum"]) == R.scenes_checksum(scenes), "synthetic scenes differ from the ones the fixture was made on"
    assert int(z["seed"]) == R.SEED and int(z["draw_seed"]) == R.DRAW_SEED and int(z["k"]) == R.K
    assert [tuple(s) for s in z["shapes"]] == R.SHAPES and list(z["order"]) == R.ORDER
    return z, scenes


def host_scenes(scenes, **kw):
    p = dict(R.PARAMS, **kw)
    return D.DeviceScenes(**{k: [s[k] for s in scenes] for k in ("lr_dem", "hr_dem", "image", "mask", "canopy")}, device="cpu", **p)


def test_host_draws_equal_the_reference_meta(g11):
    z, scenes = g11
    S = host_scenes(scenes)
    for rng in (np.random.RandomState(R.DRAW_SEED), None):
        if rng is None:
            np.random.seed(R.DRAW_SEED)            # default: numpy's global stream, as the reference draws
        rows, sides, metas = D.RandomCropBatches(S, 2, R.K, rng=rng, sampler=R.ORDER).draw(R.ORDER)
        assert sides == [R.K] * len(R.ORDER)
        for j, (s, m) in enumerate(zip(R.ORDER, metas)):
            a = m["augmentation"]
            assert m["id"] == str(s)
            assert tuple(m["bbox"]) == tuple(z[f"r{j}_bbox"]), j
            assert [a["rot90"], a["flip_lr"], a["flip_ud"]] == list(z[f"r{j}_aug"]), j
            assert np.float32(m["base"]) == z[f"r{j}_base"]
            assert rows[j, 4] == np.float32(z[f"r{j}_base"]).view(np.int32)
            assert rows[j, 3] == D.d4_code(*a.values())
            if R.SHAPES[s] == (R.K, R.K):          # the no-crop rule: the whole scene, no crop draw
                assert tuple(m["bbox"]) == (0, 0, R.K, R.K) and rows[j, 1] == rows[j, 2] == 0
            else:
                assert tuple(rows[j, 1:3]) == tuple(m["bbox"][:2])


def test_restatement_reproduces_the_fixture(g11):
    z, scenes = g11
    rand = R.random_pass(scenes, R.PARAMS, R.K, R.ORDER, np.random.RandomState(R.DRAW_SEED))
    tile = R.tile_pass(scenes, R.PARAMS, R.K, R.TILE_N, R.TILE_SCENES)
    for prefix, res in (("r", rand), ("t", tile)):
        for j, (out, base, bbox, aug) in enumerate(res):
            assert tuple(z[f"{prefix}{j}_bbox"]) == bbox
            for kind, v in out.items():
                assert np.array_equal(v, z[f"{prefix}{j}_{kind}"]), (prefix, j, kind)


def test_tile_batches_meta_equal_the_reference(g11):
    z, scenes = g11
    S = host_scenes([scenes[i] for i in R.TILE_SCENES])
    T = D.TileCropBatches(S, 4, R.K, R.TILE_N)
    assert len(T) == 5 and T.rows.shape == (18, 8)
    for j, m in enumerate(T.metas):
        assert tuple(m["bbox"]) == tuple(z[f"t{j}_bbox"]) and m["augmentation"]["rot90"] == 0
        x0, y0 = m["bbox"][:2]
        assert tuple(T.rows[j, 1:4]) == (y0, x0, 0)


@pytest.mark.parametrize("k", [5, 6])
def test_all_sixteen_d4_codes_invert_the_reference_composition(k):
    a = np.arange(k * k * 2).reshape(k, k, 2)          # no symmetry: every entry distinct
    for angle in range(4):
        for lr in (False, True):
            for ud in (False, True):
                code = D.d4_code(angle, lr, ud)
                assert np.array_equal(R.gather(a, 0, 0, k, code), R.d4(a, angle, lr, ud)), (angle, lr, ud)
    codes = {D.d4_code(a_, l_, u_) for a_ in range(4) for l_ in (0, 1) for u_ in (0, 1)}
    assert codes == set(range(16))


def test_d4_gather_inside_a_larger_scene():
    rs = np.random.RandomState(3)
    scene = rs.randint(0, 1000, (41, 37, 3))
    for code in range(16):
        y0, x0, k = 5, 2, 29
        ref = R.d4(scene[y0:y0 + k, x0:x0 + k], code >> 2, code & 2, code & 1)
        assert np.array_equal(R.gather(scene, y0, x0, k, code), ref), code


@pytest.mark.parametrize("seed", [None, 11])
def test_default_sampler_is_the_shuffling_dataloader_order(seed):
    n, B = 23, 4
    order = []
    loader = []
    for gen_order in (True, False):
        if seed is None:
            torch.manual_seed(5)
            g = None
        else:
            g = torch.Generator().manual_seed(seed)
        if gen_order:
            s = D.ShuffleOrder(n, g)
            order = [list(s) for _ in range(3)]
        else:
            dl = torch.utils.data.DataLoader(list(range(n)), batch_size=B, shuffle=True, generator=g, num_workers=0,
                                             drop_last=True, collate_fn=lambda b: b)
            loader = [[i for b in dl for i in b] for _ in range(3)]
    for e in range(3):
        assert order[e][:len(loader[e])] == loader[e] and sorted(order[e]) == list(range(n))
    assert order[0] != order[1]


def test_preload_checks():
    scenes = R.make_scenes([(40, 40), (36, 36)])
    with pytest.raises(NotImplementedError):
        host_scenes(scenes, coord="global")
    with pytest.raises(NotImplementedError):
        host_scenes(scenes, normalize=["image"])
    bad = [dict(s) for s in scenes]
    bad[1]["hr_dem"] = bad[1]["hr_dem"].copy()
    bad[1]["hr_dem"][3, 4, 0] = bad[1]["lr_dem"].min() - 90.0      # below base + elev_min + 1: log domain broken
    with pytest.raises(AssertionError):
        host_scenes(bad)
    with pytest.raises(AssertionError):
        host_scenes(scenes, relative=False, elev_max=300)          # scaled values above 1
    ok = host_scenes(scenes, relative=False, elev_min=0, elev_max=1000)
    assert ok.base == [0, 0] and ok.flags == D.LOG | D.SCALE_MASK
    S = host_scenes(R.make_scenes([(40, 30)]))
    with pytest.raises(ValueError):                                # not cropped (k > w) and not square: cannot be stacked
        D.RandomCropBatches(S, 1, 35, sampler=[0]).draw([0])


def test_batch_make_rejects_bad_arguments_without_a_gpu():
    from jspsr_amd import _lib
    lib = _lib.load()
    fake = 0x10000

    def call(src=None, nbytes=None, out=None, ch=None, coff=None, pitch=None, scenes=fake, n_scenes=1, samples=fake, B=2, k=32,
             flags=0, lo=-80.0, hi=933.0, mask_div=16):
        def arr(t, v, d):
            a = (t * 6)()
            for i, x in enumerate(v if v is not None else d):
                a[i] = x
            return a
        return lib.jspsr_batch_make(arr(ctypes.c_void_p, src, [fake] * 5 + [0]), arr(ctypes.c_longlong, nbytes, [1 << 20] * 6),
                                    arr(ctypes.c_void_p, out, [fake] * 6), arr(ctypes.c_int, ch, [1, 1, 3, 15, 1, 2]),
                                    arr(ctypes.c_int, coff, [0] * 6), arr(ctypes.c_int, pitch, [1, 1, 3, 15, 1, 2]), scenes,
                                    n_scenes, samples, B, k, flags, lo, hi, mask_div, None)

    assert lib.jspsr_batch_make(None, None, None, None, None, None, None, 1, None, 1, 32, 0, 0.0, 1.0, 16, None) == -1
    assert call(scenes=None) == -1 and call(samples=None) == -1
    assert call(B=0) == -1 and call(k=0) == -1 and call(n_scenes=0) == -1
    assert call(lo=10.0, hi=10.0) == -1 and call(mask_div=0) == -1 and call(flags=64) == -1
    assert call(flags=4 | 16) == -1                                # two image ranges at once
    assert call(ch=[1, 1, 3, 17, 1, 2]) == -1                      # more than 16 channels
    assert call(ch=[2, 1, 3, 15, 1, 2]) == -1                      # a DEM has one channel
    assert call(ch=[1, 1, 3, 15, 1, 3]) == -1                      # coord has two
    assert call(pitch=[1, 1, 3, 14, 1, 2]) == -1                   # the channels leave the output
    assert call(coff=[0, 0, -1, 0, 0, 0]) == -1
    assert call(src=[fake, 0, fake, fake, fake, 0]) == -1          # a present kind without a store
    assert call(out=[0] * 6) == -1                                 # no output at all
    assert b"batch_make" in lib.jspsr_last_error()
    assert call(out=[fake + 2] + [fake] * 5) == -2                 # output not 4-byte aligned
    assert call(src=[fake + 1] + [fake] * 4 + [0]) == -2           # store not 4-byte aligned
