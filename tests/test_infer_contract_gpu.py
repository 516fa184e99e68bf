"""K13 on the MI355X, the edges of its contract (include/jspsr_hip.h): what `jspsr_scene_prepare` does with a map entry
outside its scene, a sample row naming no scene and a scene table that leaves the store -- it writes NaN there and reads
nothing, the rest of the launch is untouched -- and the ordering of the cached uploads (maps, sample tables) when their
first use and the next one are on two streams.  Everything here is compared with ==."""
import copy

import numpy as np
import pytest
import torch

from jspsr_amd import infer as I
from tests import batches_ref as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ("lr_dem", "image", "mask", "canopy", "coord")
SENTINEL = -7.0


def store(shapes, seed):
    scenes = B.make_scenes(shapes, seed=seed)
    p = {k: v for k, v in B.PARAMS.items() if k != "label_range"}
    return I.InferenceScenes(coord="local", device=DEV, **{k: [s[k] for s in scenes] for k in KINDS[:4]}, **p)


def sample_table(Sc, scene_of_sample):
    base = [np.float32(Sc.base[min(max(s, 0), len(Sc) - 1)]).view(np.int32) for s in scene_of_sample]
    return torch.tensor([[s, b] for s, b in zip(scene_of_sample, base)], dtype=torch.int32, device=DEV)


def launch(Sc, table, rows, cols):
    """One raw launch into channel slices of a sentinel-filled tensor: a spare channel on either side of every sample."""
    C = sum(Sc.channels[k] for k in KINDS)
    view = torch.full((table.shape[0], C + 2, len(rows), len(cols)), SENTINEL, device=DEV)
    outs, c0 = {}, 1
    for k in KINDS:
        outs[k] = (view, c0)
        c0 += Sc.channels[k]
    as_dev = lambda m: torch.as_tensor(np.asarray(m, dtype=np.int32), device=DEV)      # noqa: E731
    I.launch_prepare(Sc, table, as_dev(rows), as_dev(cols), len(rows), len(cols), outs)
    assert bool((view[:, 0] == SENTINEL).all()) and bool((view[:, C + 1] == SENTINEL).all())
    return view[:, 1:C + 1]


@pytest.mark.parametrize("shape,n,multiple", [((40, 40), 12, 8), ((9, 7), 6, 1)])      # 16-byte stores / scalar stores
def test_prepare_writes_nan_for_map_entries_outside_the_scene(shape, n, multiple):
    H, W = shape
    Sc = store([shape] * 2, seed=31)
    rows, cols, _, _ = I.frame_maps(H, W, n, multiple)
    table = sample_table(Sc, [1, 0])
    good = launch(Sc, table, rows, cols)
    assert bool(torch.isfinite(good).all())
    bad_rows, bad_cols = rows.copy(), cols.copy()
    bad_rows[[0, 3, len(rows) - 1]] = (-1, H, 2 ** 31 - 1)
    bad_cols[[1, 2, len(cols) - 1]] = (W, -1, -2 ** 31)
    got = launch(Sc, table, bad_rows, bad_cols)
    nan = torch.zeros(good.shape[2:], dtype=torch.bool, device=DEV)
    nan[[0, 3, len(rows) - 1], :] = True
    nan[:, [1, 2, len(cols) - 1]] = True
    assert bool(torch.isnan(got[:, :, nan]).all())                             # every kind, coord included
    assert torch.equal(got[:, :, ~nan], good[:, :, ~nan])                      # and nothing else moved


def test_prepare_writes_nan_for_a_sample_that_names_no_scene():
    Sc = store([(37, 53)] * 2, seed=32)
    rows, cols, _, _ = I.frame_maps(37, 53, 5, 8)
    good = launch(Sc, sample_table(Sc, [1, 0, 1, 0]), rows, cols)
    got = launch(Sc, sample_table(Sc, [1, len(Sc), -1, 0]), rows, cols)        # scene = n_scenes, scene < 0
    assert bool(torch.isnan(got[1:3]).all())
    assert torch.equal(got[0], good[0]) and torch.equal(got[3], good[3])


def test_prepare_writes_nan_for_a_scene_that_leaves_its_store():
    """The last scene's extent moved one pixel past the end of the store: no raster of it is read.  `coord` has no store;
    it needs H, W > 1 only."""
    Sc = store([(40, 40)] * 2, seed=33)
    rows, cols, _, _ = I.frame_maps(40, 40, 0, 8)
    table = sample_table(Sc, [0, 1])
    good = launch(Sc, table, rows, cols)
    moved = copy.copy(Sc)
    moved.scene_table = Sc.scene_table.clone()
    moved.scene_table[1, 0] += 1
    got = launch(moved, table, rows, cols)
    c_coord = sum(Sc.channels[k] for k in KINDS[:4])
    assert torch.equal(got[0], good[0])
    assert bool(torch.isnan(got[1, :c_coord]).all()) and torch.equal(got[1, c_coord:], good[1, c_coord:])
    moved.scene_table[1] = torch.tensor([1600, 1, 40], device=DEV)            # a one-row scene has no local coordinates
    got = launch(moved, table, np.zeros(40, np.int32), cols)
    assert bool(torch.isnan(got[1, c_coord:]).all()) and bool(torch.isfinite(got[1, :c_coord]).all())


def test_cached_uploads_are_ordered_for_a_second_stream():
    """First use on stream A, queued behind other work, the next use at once on stream B, both give the right tensors; and
    the caches stay bounded.  A smoke test of the two-stream path, not a proof of the ordering: whether B would have read
    early without the event is down to timing, so code without it may pass here too."""
    Sc = store([(40, 40)] * 3, seed=34)
    I._MAPS.clear()
    a, b = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    busy = torch.zeros(64 * 1024 * 1024, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        for _ in range(30):                                                   # a few ms in front of the uploads
            busy.add_(1.0)
        first, _ = I.prepare(Sc, [2, 0, 1], 12, 8, concat=True)
    with torch.cuda.stream(b):
        second, fr = I.prepare(Sc, [2, 0, 1], 12, 8, concat=True)
    torch.cuda.synchronize()
    want, _ = I.prepare(Sc, [2, 0, 1], 12, 8, concat=True)
    torch.cuda.synchronize()
    assert (fr.Hp, fr.Wp) == (64, 64) and bool(torch.isfinite(want[0]).all())
    assert torch.equal(first[0], want[0]) and torch.equal(second[0], want[0])
    assert len(I._MAPS) == 1
    for h in range(20, 20 + I._CACHE_LIMIT + 2):                             # uploads only: no kernel launch
        I._device_maps(h, 16, 0, 1, Sc.device)
        assert len(I._MAPS) <= I._CACHE_LIMIT
    I._MAPS.clear()
