"""GPU: the feather merges -- jspsr_tiles_merge_f32 (K8), jspsr_scenes_assemble_f32 (K12a) and jspsr_scene_merge_windows
(K15), three kernels on the inlines of csrc/scene_finish.h -- on what the package's own callers never reach: square covers deeper
than two tiles, mosaics at misaligned and refused offsets of a pooled buffer, the n_x = 1 bypass with a border and a stride
given, and the ramp cover and the table cover on the same tiles.

The restatement is numpy float32, one rounding per operation, from the formulas of include/jspsr_hip.h: a tile loses
border_px per side, is multiplied by its column weights, then by its row weights, and is added to the mosaic, tile by tile
in row-major order from a mosaic of zeros; the weight of position j of the tile at cover position pos is 1, ramp[p - 1 - j]
over the first p positions where a tile precedes it, ramp[j - (w_l_c - p)] over the last p where one follows, the later
rule winning where both apply.  Metres: clamp to [0, 1] (a NaN stays), v * span + lo or exp(v * log_span) + lo, + base.
Comparisons are by bytes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jspsr_amd import _lib
from jspsr_amd import metrics as M
from jspsr_amd import tiles as T
from jspsr_amd.cover import plan_cover

F32 = np.float32
COVERS = [(8, 1, 2, 4),     # w_l_c 6, p 4, mosaic 12 x 12: three tiles deep at Y = 4..7, 16-byte stores
          (9, 1, 2, 4)]     # w_l_c 7, p 5, mosaic 13 x 13: four deep at Y = 6, scalar tail
CANARY = F32(-777.25)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sides(k, b, s, n_x):
    w_l_c = k - 2 * b
    return w_l_c, s * (n_x - 1) + w_l_c, w_l_c - s


def _weights(ramp, w_l_c, p, n_x, pos):
    w = np.ones(w_l_c, F32)
    for j in range(w_l_c):
        if pos > 0 and j < p:
            w[j] = ramp[p - 1 - j]
        if pos < n_x - 1 and j >= w_l_c - p:
            w[j] = ramp[j - (w_l_c - p)]
    return w


def merge_ref(m, ramp, k, b, s, n_x):
    """m (n_x * n_x, k, k) float32 -> the mosaic, float32."""
    w_l_c, w_h_c, p = _sides(k, b, s, n_x)
    out = np.zeros((w_h_c, w_h_c), F32)
    with np.errstate(invalid="ignore"):
        for r in range(n_x):
            for c in range(n_x):
                wy, wx = _weights(ramp, w_l_c, p, n_x, r), _weights(ramp, w_l_c, p, n_x, c)
                t = m[r * n_x + c, b:k - b, b:k - b]
                term = ((t * wx[None, :]).astype(F32) * wy[:, None]).astype(F32)
                out[s * r:s * r + w_l_c, s * c:s * c + w_l_c] += term
    return out


def metres_ref(v, elev_log, elev_min, elev_max, base):
    """clamp -> descale_data -> + base in float32.  Linear: numpy alone.  Log: the exponential is the device library's, so
    descale_data is jspsr_elev_scale_f32 -- the header's own statement of the contract -- held to numpy's within 5 ulp: an
    exponential of at most ~2 ulp on either side and the half ulp of each sum."""
    with np.errstate(invalid="ignore"):
        c = np.where(v < 0, F32(0), np.where(v > 1, F32(1), v)).astype(F32)
        lo, span, log_span = F32(elev_min), F32(elev_max - elev_min), F32(np.log(elev_max - elev_min))
        if elev_log:
            d = M.descale_data(_dev(c), elev_min, elev_max, True).cpu().numpy()
            host = (np.exp((c * log_span).astype(F32)).astype(F32) + lo).astype(F32)
            assert np.allclose(d, host, rtol=6e-7, atol=0, equal_nan=True)
        else:
            d = ((c * span).astype(F32) + lo).astype(F32)
        return (d + F32(base)).astype(F32)


def _tiles_merge(lib, m, ramp, k, b, s, n_x):
    w_h_c = _sides(k, b, s, n_x)[1]
    out = torch.full((w_h_c, w_h_c), float(CANARY), device="cuda")
    d_m, d_ramp = _dev(m), _dev(ramp)                                 # named: alive until the result is back
    n0 = lib.jspsr_launch_count(b"tiles_merge")
    assert lib.jspsr_tiles_merge_f32(d_m.data_ptr(), d_ramp.data_ptr(), out.data_ptr(), n_x, k, b, s, _stream()) == 0
    assert lib.jspsr_launch_count(b"tiles_merge") == n0 + 1
    got = out.cpu().numpy()
    del d_m, d_ramp
    return got


def _case(k, b, s, n_x, S=1, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(1000 * k + S)
    p = _sides(k, b, s, n_x)[2]
    ramp = rng.uniform(0.1, 0.9, p).astype(F32)                       # strictly inside (0, 1)
    m = rng.uniform(lo, hi, (S * n_x * n_x, k, k)).astype(F32)
    return m, ramp


@pytest.mark.parametrize("k,b,s,n_x", COVERS)
def test_tiles_merge_on_covers_deeper_than_two_tiles(k, b, s, n_x):
    lib = _lib.load()
    w_l_c, w_h_c, p = _sides(k, b, s, n_x)
    depth = np.zeros(w_h_c, int)
    for t in range(n_x):
        depth[s * t:s * t + w_l_c] += 1
    assert depth.max() == (3 if k == 8 else 4)
    m, ramp = _case(k, b, s, n_x)
    got = _tiles_merge(lib, m, ramp, k, b, s, n_x)
    assert got.tobytes() == merge_ref(m, ramp, k, b, s, n_x).tobytes()

    # no zero-weight skip: a NaN tile shows at exactly the pixels it covers, whatever the ramp holds
    ramp[1] = 0
    r, c = 1, 2
    m[r * n_x + c] = np.nan
    got = _tiles_merge(lib, m, ramp, k, b, s, n_x)
    assert got.tobytes() == merge_ref(m, ramp, k, b, s, n_x).tobytes()
    covered = np.zeros((w_h_c, w_h_c), bool)
    covered[s * r:s * r + w_l_c, s * c:s * c + w_l_c] = True
    assert np.array_equal(np.isnan(got), covered)


def _assemble(lib, m, base, ramp, buf, off, S, n_x, k, b, s, elev_log, elev_min, elev_max):
    out, d_m, d_base, d_off = _dev(buf), _dev(m), _dev(np.asarray(base, F32)), _dev(np.asarray(off, np.int64))
    d_ramp = _dev(ramp) if ramp is not None else None                 # all named: alive until the result is back
    n0 = lib.jspsr_launch_count(b"scenes_assemble")
    rc = lib.jspsr_scenes_assemble_f32(d_m.data_ptr(), d_base.data_ptr(), d_ramp.data_ptr() if ramp is not None else None,
                                       out.data_ptr(), d_off.data_ptr(), buf.size, S, n_x, k, b, s, int(elev_log),
                                       ctypes.c_double(elev_min), ctypes.c_double(elev_max), _stream())
    assert rc == 0 and lib.jspsr_launch_count(b"scenes_assemble") == n0 + 1
    got = out.cpu().numpy()
    del d_m, d_base, d_off, d_ramp
    return got


@pytest.mark.parametrize("elev_log", [False, True])
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("k,b,s,n_x", COVERS)
def test_scenes_assemble_at_misaligned_and_refused_offsets(k, b, s, n_x, aligned, elev_log):
    lib = _lib.load()
    S, elev_min, elev_max, base = 3, 2.5, 1800.0, [100.5, -3.25, 7.0]
    total = _sides(k, b, s, n_x)[1] ** 2
    m, ramp = _case(k, b, s, n_x, S, -0.2, 1.2)
    m[5, 3, 3], m[n_x * n_x + 2, 2, 4] = np.nan, -0.0
    # misaligned starts and a refused scene; aligned: mosaic 0 on a 16-byte boundary, mosaic 1 off it, mosaic 2 past the end
    off = [0, total + 1, 2 * total] if aligned else [1, 1 + total + 2, -1]
    buf = np.full(off[1] + total + 3, CANARY, F32)
    got = _assemble(lib, m, base, ramp, buf, off, S, n_x, k, b, s, elev_log, elev_min, elev_max)
    want = buf.copy()
    for sc in range(2):
        mm = metres_ref(m[sc * n_x * n_x:(sc + 1) * n_x * n_x], elev_log, elev_min, elev_max, base[sc])
        want[off[sc]:off[sc] + total] = merge_ref(mm, ramp, k, b, s, n_x).ravel()
    assert np.isnan(want).sum() == 1 and (want == CANARY).sum() == buf.size - 2 * total
    assert got.tobytes() == want.tobytes()           # the mosaics, the canaries around them, nothing of the refused scene


@pytest.mark.parametrize("elev_log,elev_min,base", [(False, -0.0, -0.0), (True, 2.5, 100.5)])
def test_scenes_assemble_single_tile_is_the_uncropped_tile_in_metres(elev_log, elev_min, base):
    lib = _lib.load()
    k, elev_max = 5, 1800.0
    m = np.random.default_rng(5).uniform(-0.2, 1.2, (2, k, k)).astype(F32)
    m[0, 0, 0], m[0, 1, 1], m[1, 2, 2] = -0.0, 0.0, np.nan
    buf = np.full(2 * k * k + 3, CANARY, F32)
    got = _assemble(lib, m, [base, base], None, buf, [1, 2 + k * k], 2, 1, k, 1, 3, elev_log, elev_min, elev_max)
    want = buf.copy()
    for sc, o in enumerate([1, 2 + k * k]):
        want[o:o + k * k] = metres_ref(m[sc], elev_log, elev_min, elev_max, base).ravel()
    if not elev_log:
        assert np.signbit(want[1]) and not np.signbit(want[1 + k + 1])      # -0.0 stays -0.0: written, not accumulated
    assert got.tobytes() == want.tobytes()


def test_the_table_cover_and_the_ramp_cover_merge_the_same_tiles_alike():
    lib = _lib.load()
    full, k, n = 70, 32, 9
    cover = plan_cover(full, full, k, 13)
    assert list(cover.ox) == [0, 19, 38] and list(cover.oy) == [0, 19, 38] and T.get_tile(full, k, n) == (19, n)
    tiles = torch.randn(n, 1, k, k, generator=torch.Generator().manual_seed(70)).cuda()
    want = T.merge_tiles(tiles, full, 0.0)
    tabs = [_dev(a) for a in (cover.wy, cover.wx, cover.lo_y, cover.lo_x, cover.oy, cover.ox, np.zeros((1, 2), np.int32))]
    out = torch.empty((1, full, full), device="cuda")
    rc = lib.jspsr_scene_merge_windows(0, tiles.data_ptr(), *[t.data_ptr() for t in tabs], out.data_ptr(), 1, 3, 3, k, k, full,
                                       full, 0, 0, ctypes.c_double(0.0), ctypes.c_double(1.0), _stream())
    assert rc == 0
    assert out[0].cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
