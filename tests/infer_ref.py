"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the steps of the reference's whole-scene inference for the K13 tests
(jspsr_amd/infer.py, csrc/scene.hip): `add_padding` / `remove_padding` (utils/utils.py:1501-1531) by slicing, as the
reference writes them, then `ToTensor` (data/data_utils.py:217-312) through tests/batches_ref.py's numpy expressions
(DeviceScenes.scale_dem's, `/ 255`, `(i + 1) / mask_div`).  Also the frozen inputs of tests/golden/g14_infer.npz
(tools/gen_golden_infer.py), regenerated from their seed.  CPU only.
"""
from __future__ import annotations

import numpy as np

from tests import batches_ref as B

SEED = 1414
PAD_CASES = [(40, 40, 3, 12), (37, 53, 15, 5), (9, 7, 1, 6)]          # (H, W, C, n) of the fixture's add_padding calls
CAL_PAD_SIDES = [37, 40, 100, 334, 512, 600, 601]
DEM_PAD = 12                                                          # the 40 x 40 DEM is padded by 12 before scale_data
ELEV_MIN, ELEV_MAX = -80, 933


def golden_inputs():
    """The fixture's inputs from the frozen legacy stream: an image-like raster, a one-hot mask, a tiny fp32 raster and a
    40 x 40 DEM.  -> ([array per PAD_CASES entry], dem)"""
    rs = np.random.RandomState(SEED)
    (h0, w0, c0, _), (h1, w1, c1, _), (h2, w2, c2, _) = PAD_CASES
    img = rs.randint(0, 256, (h0, w0, c0)).astype(np.uint8)
    msk = (rs.randint(0, c1, (h1, w1))[..., None] == np.arange(c1)).astype(np.uint8)
    tiny = rs.uniform(-50, 900, (h2, w2, c2)).astype(np.float32)
    yy, xx = np.mgrid[0:40, 0:40].astype(np.float32)
    dem = (250 + 60 * np.sin(yy / 7) * np.cos(xx / 9) + rs.uniform(0, 90, (40, 40))).astype(np.float32)[..., None]
    return [img, msk, tiny], dem


def inputs_checksum() -> str:
    arrays, dem = golden_inputs()
    return B.checksum(arrays + [dem])


def add_padding(img: np.ndarray, n: int) -> np.ndarray:
    """The mirrored border, slice for slice (utils/utils.py:1501-1520): HWC in, float32 HWC out.  The columns first; then
    the top strip from the first n padded rows, and the bottom strip from the n rows that END one row above the last image
    row's successor -- rows [-2n-1, -n-1) of the padded array -- reversed."""
    h, w, c = img.shape
    out = np.empty((h + 2 * n, w + 2 * n, c), np.float32)
    out[n:n + h, n:n + w] = img
    out[n:n + h, :n] = img[:, :n][:, ::-1]
    out[n:n + h, -n:] = img[:, -n:][:, ::-1]
    out[:n] = out[n:2 * n][::-1]
    out[-n:] = out[-2 * n - 1:-n - 1][::-1]
    return out


def remove_padding(img: np.ndarray, n: int) -> np.ndarray:
    h, w, _ = img.shape
    return img[n:h - n, n:w - n]


def frame(img: np.ndarray, n: int, multiple: int = 1) -> np.ndarray:
    """add_padding, then the frame brought to a multiple: the bottom rule continued over the extra rows (frame row Y takes
    image row 2H + n - 2 - Y) and the right rule over the extra columns (image column 2W + n - 1 - X).  The reference has
    no such step (its model fails on other sizes); this is the package's documented rule, written with slices."""
    h, w, _ = img.shape
    p = add_padding(img, n) if n > 0 else img.astype(np.float32)
    eh, ew = (-(h + 2 * n)) % multiple, (-(w + 2 * n)) % multiple
    if eh:
        first = 2 * h + n - 2 - (h + 2 * n) + n                      # padded row holding the first extra row's image row
        p = np.concatenate([p, p[first - eh + 1:first + 1][::-1]], axis=0)
    if ew:
        first = 2 * w + n - 1 - (w + 2 * n) + n
        p = np.concatenate([p, p[:, first - ew + 1:first + 1][:, ::-1]], axis=1)
    return p


def model_inputs(scene: dict, params: dict, n: int, multiple: int = 1, base=None) -> dict:
    """upscale_dem's input side for one decoded scene {kind: HWC array} (a "coord" entry made by
    batches_ref.local_coord is padded like any raster): pad every raster, then ToTensor -> {kind: fp32 CHW}."""
    if base is None:
        base = np.min(scene["lr_dem"]) if params["relative"] else 0
    padded = {}
    for kind, a in scene.items():
        f = frame(a, n, multiple)
        padded[kind] = f.astype(np.uint8) if kind in ("image", "mask", "canopy") else f      # ToTensor: tmp.astype(np.uint8)
    return B.to_tensor(padded, params, base)
