"""Numpy restatement of the reference's training-sample chain for the K9 tests (jspsr_amd/data.py, csrc/batch.hip):
RandomCrop -> RandomFlipRotate90 -> ToTensor (data/data_utils.py:9-312) and TileCrop's cover, one sample at a time, with
the same numpy dtypes the reference computes in (NumPy 2 promotion).  Also the synthetic scenes of the g11 fixture
(tools/gen_golden_batches.py), regenerated from their seed.
"""
from __future__ import annotations

import hashlib

import numpy as np

SEED = 2024                 # scene contents
DRAW_SEED = 7               # np.random.seed before the draws
K = 32
SHAPES = [(70, 70), (96, 80), (48, 48), (32, 32)]       # scene 3 takes the no-crop rule (k == h == w)
ORDER = [0, 1, 2, 3, 1, 0, 2, 1, 3, 0]                  # sample order of the random pass
TILE_SCENES, TILE_N = [0, 1], 9
PARAMS = dict(relative=True, elev_min=-80, elev_max=933, elev_log=True, scale_mask=True, mask_channel=list(range(15)),
              image_range=None, label_range=None)
KIND_ORDER = ("lr_dem", "image", "hr_dem", "coord", "mask", "canopy")       # DFC30.__getitem__'s key order


def make_scenes(shapes=SHAPES, seed=SEED, mask_c=15, coord=False):
    """Decoded scenes as DFC30.__getitem__ holds them: smooth fp32 DEMs around 150-400 m, uint8 RGB, a one-hot uint8 mask
    of mask_c classes, uint8 canopy heights 0..68."""
    rs = np.random.RandomState(seed)
    out = []
    for h, w in shapes:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        z = 250 + 60 * np.sin(yy / 7 + rs.uniform(0, 6)) * np.cos(xx / 9) + rs.uniform(0, 90, (h, w)).astype(np.float32)
        lr = z.astype(np.float32)[..., None]
        hr = (z + rs.uniform(-20, 20, (h, w))).astype(np.float32)[..., None]
        cls = rs.randint(0, mask_c, (h, w))
        s = {"lr_dem": lr, "hr_dem": hr, "image": rs.randint(0, 256, (h, w, 3)).astype(np.uint8),
             "mask": (cls[..., None] == np.arange(mask_c)).astype(np.uint8),
             "canopy": rs.randint(0, 69, (h, w, 1)).astype(np.uint8)}
        if coord:
            s["coord"] = local_coord(h, w)
        out.append(s)
    return out


def checksum(arrays) -> str:
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def scenes_checksum(scenes) -> str:
    return checksum([s[k] for s in scenes for k in sorted(s)])


def local_coord(h, w):
    """DFC30._gen_coord(coord_mode='local'), dfc30.py:292-307: channel 0 row / (H-1), channel 1 col / (W-1)."""
    xx, yy = np.mgrid[0:h, 0:w]
    return np.concatenate([(xx.astype(np.float32) / (h - 1))[..., None], (yy.astype(np.float32) / (w - 1))[..., None]], axis=2)


def draw(rs, h, w, k, augment=True):
    """One sample's draws in the reference's order: ((y0, x0) or None when the crop is skipped, (angle, lr, ud))."""
    crop = None
    if not (k > h or k > w or k == h == w):
        crop = (int(rs.randint(0, h - k - 1)), int(rs.randint(0, w - k - 1)))
    aug = (0, False, False)
    if augment and rs.random_sample() < 0.5:
        aug = (int(rs.choice([1, 2, 3])), bool(rs.choice([True, False])), bool(rs.choice([True, False])))
    return crop, aug


def d4(a, angle, lr, ud):
    """RandomFlipRotate90 on an HWC array (data_utils.py:26-28)."""
    a = np.rot90(a, angle)
    a = np.fliplr(a) if lr else a
    return np.flipud(a) if ud else a


def d4_source(code, k, i, j):
    """The kernel's inverse map (csrc/batch.hip:d4_source): output (i, j) -> crop (sy, sx); works on index arrays."""
    i2 = k - 1 - i if code & 1 else i
    j2 = k - 1 - j if code & 2 else j
    angle = code >> 2
    if angle == 0:
        return i2, j2
    if angle == 1:
        return j2, k - 1 - i2
    if angle == 2:
        return k - 1 - i2, k - 1 - j2
    return k - 1 - j2, i2


def gather(a, y0, x0, k, code):
    """out[y][x] = a[y0 + sy][x0 + sx] over the k x k output, by the inverse map (HWC in, HWC out)."""
    i, j = np.mgrid[0:k, 0:k]
    sy, sx = d4_source(code, k, i, j)
    return a[y0 + sy, x0 + sx]


def scale_dem(data, p, base):
    data = data.astype(np.float32)
    if base != 0:
        data = data - base
    if p["elev_log"]:
        assert np.min(data) - p["elev_min"] >= 1
        return np.log(data - p["elev_min"]) / np.log(p["elev_max"] - p["elev_min"]) + 1e-8
    return (data - p["elev_min"]) / (p["elev_max"] - p["elev_min"])


def to_tensor(sample, p, base):
    """ToTensor.__call__ (data_utils.py:217-283) on HWC arrays -> {kind: fp32 CHW}; torchvision's to_tensor on uint8 is
    CHW float / 255 in fp32."""
    out = {}
    for kind, a in sample.items():
        if kind == "image":
            t = np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
            if p["image_range"] == "[-1, 1]":
                t = np.float32(2.0) * t - np.float32(1.0)
            elif p["image_range"] == "[0, 255]":
                t = t / np.float32(255.0)
            out[kind] = t
            continue
        t = a.transpose((2, 0, 1)).astype(np.float32)
        if "dem" in kind:
            t = scale_dem(t, p, base)
            rng = p["label_range"] if kind == "hr_dem" else p["image_range"]
            if rng == "[-1, 1]":
                t = t * 2 - 1
        if kind == "mask" and p["scale_mask"]:
            for i in range(t.shape[0]):
                t[i] = t[i] * (i + 1) / (len(p["mask_channel"]) + 1)
        if kind == "canopy":
            t = t / 68
        out[kind] = np.ascontiguousarray(t).astype(np.float32)
    return out


def sample(scene, p, k, crop, aug):
    """One training sample: crop (or not), D4, ToTensor; scene may hold 'coord' already."""
    base = np.min(scene["lr_dem"]) if p["relative"] else 0
    s = {}
    for kind in KIND_ORDER:
        if kind not in scene:
            continue
        a = scene[kind]
        if crop is not None:
            a = a[crop[0]:crop[0] + k, crop[1]:crop[1] + k, :]
        if aug[0]:
            a = d4(a, *aug)
        s[kind] = a
    return to_tensor(s, p, base), base


def random_pass(scenes, p, k, order, rs, augment=True):
    """[(outputs, base, bbox, aug)] for the samples of `order`, the draws taken from RandomState rs."""
    res = []
    for s in order:
        h, w = scenes[s]["lr_dem"].shape[:2]
        crop, aug = draw(rs, h, w, k, augment)
        out, base = sample(scenes[s], p, k, crop, aug)
        bbox = (crop[0], crop[1], crop[0] + k, crop[1] + k) if crop else (0, 0, h, w)
        res.append((out, base, bbox, aug))
    return res


def tile_pass(scenes, p, k, n, which):
    """TileCrop over the scenes `which`, n tiles each, row-major (data_utils.py:98-168)."""
    from jspsr_amd.tiles import get_tile
    res = []
    for s in which:
        h, w = scenes[s]["lr_dem"].shape[:2]
        stride, n2 = get_tile(w, k, n)
        n_x = int(round(n2 ** 0.5))
        for t in range(n2):
            r, c = divmod(t, n_x)
            out, base = sample(scenes[s], p, k, (stride * r, stride * c), (0, False, False))
            res.append((out, base, (stride * c, stride * r, stride * c + k, stride * r + k), (0, False, False)))
    return res
