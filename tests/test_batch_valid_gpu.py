"""GPU: the validity plane of a batch (K19, jspsr_batch_valid in csrc/batch.hip) against host crops moved by np.rot90 /
fliplr / flipud in the reference's order (tests/batches_ref.d4), and `batch["valid"]` through the batch iterables."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jspsr_amd import _lib
from jspsr_amd import data as D
from tests import batches_ref as R

DEV = "cuda:0"
P = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True)
SHAPES = [(39, 47), (40, 40)]          # scene 1 starts at pixel 1833: its rows sit at every byte alignment


def rasters(shapes, seed):
    rs = np.random.RandomState(seed)
    hrs = [rs.uniform(150, 400, s).astype(np.float32)[..., None] for s in shapes]
    lrs = [h + rs.uniform(-3, 3, h.shape).astype(np.float32) for h in hrs]
    return lrs, hrs, rs


@pytest.fixture(scope="module")
def store():
    lrs, hrs, rs = rasters(SHAPES, 19)
    planes = [rs.rand(*s) < 0.6 for s in SHAPES]
    return D.DeviceScenes(lrs, hrs, device=DEV, valid=planes, **P), planes, hrs


def launches():
    return _lib.load().jspsr_launch_count(b"batch_valid")


@pytest.mark.parametrize("k", [13, 32, 37])        # no multiple of 4; exactly one LDS tile; more than one tile
def test_all_codes_at_every_scene_corner(store, k):
    S, planes, hrs = store
    rows, refs = [], []
    for s, (h, w) in enumerate(SHAPES):
        for y0, x0 in ((0, 0), (0, w - k), (h - k, 0), (h - k, w - k)):
            for code in range(16):
                rows.append([s, y0, x0, code, 0, 0, 0, 0])
                refs.append(R.d4(planes[s][y0:y0 + k, x0:x0 + k], code >> 2, bool(code & 2), bool(code & 1)))
    table = torch.tensor(rows, dtype=torch.int32, device=DEV)
    n0 = launches()
    got = S.make_valid(table, k)
    torch.cuda.synchronize()
    assert launches() == n0 + 1
    assert got.shape == (len(rows), 1, k, k) and got.dtype == torch.uint8
    want = torch.from_numpy(np.stack(refs).astype(np.uint8))[:, None]
    assert torch.equal(got.cpu(), want), [i for i in range(len(rows)) if not torch.equal(got[i].cpu(), want[i])][:8]
    # it lines up with hr_dem element for element: the same rows through jspsr_batch_make over a store whose voids are
    # marked in the raster itself (base 0, linear scaling: -32767 maps to the batch's smallest value)
    marked = [np.where(p, h[..., 0], np.float32(-32767.0))[..., None] for p, h in zip(planes, hrs)]
    T = D.DeviceScenes([np.full_like(m, 200.0) for m in marked], marked, device=DEV, hr_nodata=-32767, relative=False,
                       elev_min=-40000, elev_max=933)
    raw = torch.empty((len(rows), 1, k, k), device=DEV)
    T.make(table, k, {"hr_dem": (raw, 0)})
    assert torch.equal(raw == raw.min(), got == 0) and torch.equal(T.make_valid(table, k), got)


def test_a_row_outside_its_scene_writes_zero(store):
    S, planes, _ = store
    k = 13
    rows = [[0, 0, 0, 0], [0, 39 - k + 1, 0, 0], [0, 0, 47 - k + 1, 5], [1, -1, 0, 0], [2, 0, 0, 0], [-1, 0, 0, 0], [1, 0, 0, 16],
            [1, 40 - k, 40 - k, 15]]
    table = torch.tensor([r + [0, 0, 0, 0] for r in rows], dtype=torch.int32, device=DEV)
    got = S.make_valid(table, k).cpu()
    assert torch.equal(got[0, 0], torch.from_numpy(planes[0][:k, :k].astype(np.uint8)))
    assert not got[1:7].any()
    assert torch.equal(got[7, 0], torch.from_numpy(R.d4(planes[1][40 - k:, 40 - k:], 3, True, True).astype(np.uint8)))
    # a plane shorter than its scenes say: every row of the scene that leaves the store writes 0
    short = torch.empty((1, 1, k, k), dtype=torch.uint8, device=DEV)
    lib = _lib.load()
    one = torch.tensor([[1, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int32, device=DEV)
    plane = S.store["valid"]
    _lib.check(lib.jspsr_batch_valid(plane.data_ptr(), plane.numel() - 8, short.data_ptr(), S.scene_table.data_ptr(), 2,
                                     one.data_ptr(), 1, k, torch.cuda.current_stream().cuda_stream), "jspsr_batch_valid")
    assert not short.any()


@pytest.mark.parametrize("concat", [False, True])
def test_batches_carry_the_plane_only_for_a_store_that_has_it(concat):
    shapes = [(40, 40), (48, 48), (45, 52)]
    lrs, hrs, rs = rasters(shapes, 23)
    plain = D.DeviceScenes(lrs, hrs, device=DEV, **P)
    ones = D.DeviceScenes(lrs, hrs, device=DEV, hr_nodata=-32767, **P)              # no void: an all-ones plane
    planes = [rs.rand(*s) < 0.5 for s in shapes]
    some = D.DeviceScenes(lrs, hrs, device=DEV, valid=planes, **P)
    assert "valid" not in plain.store and bool(ones.store["valid"][:sum(h * w for h, w in shapes)].all())

    def random(S):
        return list(D.RandomCropBatches(S, 3, 32, rng=np.random.RandomState(3), sampler=[2, 0, 1, 1, 2, 0], concat=concat))

    def tiles(S):
        two = D.DeviceScenes(lrs[:2], hrs[:2], device=DEV, **P) if S is plain else \
            D.DeviceScenes(lrs[:2], hrs[:2], device=DEV, valid=None if S is ones else planes[:2], hr_nodata=-32767, **P)
        return list(D.TileCropBatches(two, 3, 32, 4, concat=concat))

    for make in (random, tiles):
        n0 = launches()
        a = make(plain)
        assert launches() == n0 and all("valid" not in b for b in a)
        b = make(ones)
        assert launches() == n0 + len(b) and len(a) == len(b)
        for x, y in zip(a, b):
            assert set(y) == set(x) | {"valid"}
            assert y["valid"].dtype == torch.uint8 and y["valid"].shape == (x["hr_dem"].shape[0], 1, 32, 32) and bool(y["valid"].all())
            for key in x:
                if isinstance(x[key], torch.Tensor):
                    assert torch.equal(x[key], y[key]), key
                else:
                    assert x[key] == y[key], key
            assert len(D.batch_pair(y, "EDSR" if concat else "JSPSR", {"lr_dem": 1})) == 4          # batch_pair keeps its 4-tuple
        c = make(some)
        for y in c:
            for i, m in enumerate(y["meta"]):
                s = int(m["id"])
                aug = m["augmentation"]
                if make is random:
                    y0, x0, y1, x1 = m["bbox"]
                else:
                    x0, y0, x1, y1 = m["bbox"]                                          # TileCrop's (x0, y0, x1, y1)
                want = R.d4(planes[s][y0:y1, x0:x1], aug["rot90"], aug["flip_lr"], aug["flip_ud"])
                assert np.array_equal(y["valid"][i, 0].cpu().numpy(), want.astype(np.uint8)), (s, m)
