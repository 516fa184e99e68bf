"""The case table of the workspace contract (tests/test_workspace_contract_gpu.py, tests/test_workspace_contract_cpu.py).

Every `jspsr_*_workspace_bytes` query of include/jspsr_hip.h promises "this many bytes are enough".  A Case names a query,
its arguments, the entries that use the workspace (forward before backward, producer before fold), the launches the census
must show, the outputs the header documents as overwritten or accumulated, and touched_bytes: the highest workspace byte
the launches address, in plain Python integers, written from the launch code (grid size x row width, region by region)
and from the header where it documents the layout.  It never calls the query.

The operands come from the generators of the existing reference modules (masked_loss_ref.pair, eval_ref's recipe); a shape
smaller than a generator's fixed indices is cut out of a larger field.  Builders issue raw ctypes calls through a context
(`ctx`) the GPU test provides: ctx.inp / ctx.out / ctx.acc make guarded arenas, ctx.ws is the workspace, ctx.call the entry.

HELD names the queries with cases here, ELSEWHERE the ones an earlier test already holds with exact bytes and a canary: the
two together are the complete list, and the CPU test fails on a query that is in neither."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

EINVAL, EALIGN = -1, -2
F32, BF16 = 0, 1


def r16(x):
    return (x + 15) // 16 * 16


def cdiv(a, b):
    return (a + b - 1) // b


def clamp(x, lo, hi):
    return max(lo, min(hi, x))


@dataclass
class Case:
    name: str
    query: str
    qargs: tuple
    run: object                 # run(ctx): makes the operands and issues the calls
    launches: dict              # census label -> count
    touched: object             # touched(*qargs) -> bytes
    branch: str                 # which branch / rounding term of the query's expression this case takes
    align: int = 16             # the workspace alignment the header documents
    bits: bool = True           # same bits on every run (no float atomics): read from the kernels, see the case's comment

    @property
    def untouched(self):        # a path that never addresses its workspace (the one-launch meters)
        return self.touched(*self.qargs) == 0


@dataclass
class Refusal:
    name: str
    query: str
    bad: tuple                  # query arguments at the documented boundary: query 0, entry `code`
    ok: tuple                   # one step inside: both accept
    run: object                 # run(ctx, qargs, alloc): the calls with `qargs`, operands sized for `alloc`
    code: int = EINVAL
    launches: dict = field(default_factory=dict)


# ---- operands --------------------------------------------------------------------------------------------------------------
def loss_pair(seed, B, H, W):
    """masked_loss_ref.pair on a field of at least 4 x 4 (its two exact zeros sit at fixed indices), cut to (B, H, W)."""
    from tests import masked_loss_ref as ML
    p, g = ML.pair(seed, (B, 1, max(H, 4), max(W, 4)))
    return np.ascontiguousarray(p[:, 0, :H, :W]), np.ascontiguousarray(g[:, 0, :H, :W])


def void_plane(seed, shape, holes=3):
    """uint8 plane, 1 = valid, with a few rectangular voids and single pixels (none when the raster is one element)."""
    rs = np.random.RandomState(seed)
    v = np.ones(shape, np.uint8)
    B, H, W = shape
    if H * W > 1:
        for _ in range(holes):
            b, y, x = rs.randint(B), rs.randint(H), rs.randint(W)
            v[b, y:y + 1 + rs.randint(max(1, H // 4)), x:x + 1 + rs.randint(max(1, W // 4))] = 0
        v[rs.randint(B), rs.randint(H), rs.randint(W)] = 0
    return v


def small_ints(seed, shape):
    """What an accumulated output holds before the call: small integers, the same in every run."""
    return np.random.RandomState(seed).randint(-3, 4, shape).astype(np.float32)


# ---- fused loss (csrc/train_step.hip) --------------------------------------------------------------------------------------
LT = 256


def loss_blocks(n):
    return clamp(cdiv(n, LT), 1, 2048)


def touched_loss(B, H, W):
    n = B * H * W
    # loss_forward: `blocks` rows of 3 floats at 0; the sign bytes, 2 per element, behind the rows rounded up to 16
    return r16(loss_blocks(n) * 3 * 4) + 2 * n


def touched_loss_valid(B, H, W):
    n = B * H * W
    blocks = loss_blocks(n)
    cnt = r16(blocks * 3 * 4)              # pcnt: `blocks` rows of 2 uint32
    nn = cnt + r16(blocks * 2 * 4)         # {N, N_g}: two int64
    return nn + 16 + 2 * n                 # sign bytes


def run_loss(ctx, B, H, W, alloc=None):
    aB, aH, aW = alloc or (B, H, W)
    p, g = loss_pair(11, aB, aH, aW)
    pp, gp = ctx.inp("pred", p), ctx.inp("gt", g)
    up = ctx.inp("grad_total", np.array([0.5], np.float32))
    losses = ctx.out("losses", (4,), np.float32)
    gpred = ctx.out("grad_pred", (aB, aH, aW), np.float32)        # "The backward writes d(Total)/d(pred) * grad_total[0]"
    ws = ctx.ws()
    c_f = ctypes.c_float
    ctx.call("jspsr_loss_forward", pp, gp, c_f(1.0), c_f(1.0), c_f(0.1), losses, ws, B, H, W, ctx.stream)
    ctx.call("jspsr_loss_backward", pp, gp, up, c_f(1.0), c_f(1.0), c_f(0.1), gpred, ws, B, H, W, ctx.stream)


def run_loss_valid(ctx, B, H, W, alloc=None):
    aB, aH, aW = alloc or (B, H, W)
    p, g = loss_pair(12, aB, aH, aW)
    v = void_plane(13, (aB, aH, aW))
    p[v == 0] = np.nan                                             # read only behind a select on the plane
    pp, gp, vp = ctx.inp("pred", p), ctx.inp("gt", g), ctx.inp("valid", v)
    up = ctx.inp("grad_total", np.array([0.5], np.float32))
    losses = ctx.out("losses", (4,), np.float32)
    gpred = ctx.out("grad_pred", (aB, aH, aW), np.float32)        # written everywhere, +0.0 at an invalid element
    ws = ctx.ws()
    c_f = ctypes.c_float
    ctx.call("jspsr_loss_valid_forward", pp, gp, vp, c_f(1.0), c_f(1.0), c_f(0.1), losses, ws, B, H, W, ctx.stream)
    ctx.call("jspsr_loss_valid_backward", pp, gp, vp, up, c_f(1.0), c_f(1.0), c_f(0.1), gpred, ws, B, H, W, ctx.stream)


LOSS_LAUNCHES = {"loss_forward": 1, "loss_finalize": 1, "loss_backward": 1}
LOSS_VALID_LAUNCHES = {"loss_valid_forward": 1, "loss_valid_finalize": 1, "loss_valid_backward": 1}
# (B, H, W): one element; 2 and 3 blocks, whose rows (24 / 36 bytes; 16 / 24 of counters) are no multiples of 16;
# 4 blocks, where no rounding term adds anything; 1 x 725 x 725 = 2054 blocks wanted, the cap of 2048 taken
LOSS_SHAPES = [((1, 1, 1), "1 block; rows rounded 12 -> 16"), ((1, 1, 257), "2 blocks; rows rounded 24 -> 32"),
               ((1, 3, 256), "3 blocks; rows rounded 36 -> 48, counters 24 -> 32"), ((2, 8, 64), "4 blocks; no rounding"),
               ((1, 725, 725), "block cap 2048")]


# ---- the loss menu and SSIM (csrc/loss_terms.hip) --------------------------------------------------------------------------
T_BERHU, T_BCE, T_NORM, T_SSIM = 1, 2, 4, 8
ST = 32                                     # SSIM tile edge


def pw_blocks(n):
    return clamp(cdiv(n, 256), 1, 2048)


def max_blocks(n):
    return clamp(cdiv(n, 256), 1, 256)


def ssim_tiles(Hm, Wm):
    return cdiv(Wm, ST) * cdiv(Hm, ST)


def touched_menu(terms, planes, H, W):
    n = planes * H * W
    off = end = 16                          # th[4]; written and read with BerHu only, but every later region sits behind it
    if not terms & T_BERHU:
        end = 0
    if terms & 7:
        end = off + max_blocks(n) * 4 if terms & T_BERHU else end       # pmax: one float per block of the max pass
        off += r16(max_blocks(n) * 4)
        end = off + pw_blocks(n) * 12       # psum: three floats per block of the sum pass
        off += r16(pw_blocks(n) * 12)
    if terms & T_SSIM:
        Hm, Wm = H - 10, W - 10
        off += r16(ssim_tiles(Hm, Wm) * planes * 4)                     # ssum: one float per (plane, tile)
        end = off + planes * Hm * Wm * 12   # alpha, beta, gamma of every map element
    return end


def valid_regions(n):
    """-> (offset of {N}, end of the K19 layout): th 16, pmax, psum, pcnt (one uint32 per block), N int64 in 16 bytes."""
    nn = 16 + r16(max_blocks(n) * 4) + r16(pw_blocks(n) * 12) + r16(pw_blocks(n) * 4)
    return nn, nn + 16


def touched_menu_valid(terms, planes, H, W):
    return valid_regions(planes * H * W)[0] + 8          # the combine kernel always writes N, the last thing of the layout


def touched_menu_valid_ssim(terms, planes, H, W, rule):
    nn, off = valid_regions(planes * H * W)
    if not terms & T_SSIM:
        return nn + 8
    Hm, Wm = H - 10, W - 10
    nbs = ssim_tiles(Hm, Wm) * planes
    off += 2 * r16(nbs * 4) + 16            # ssum, scnt, N_s
    return off + planes * Hm * Wm * 12      # the coefficient maps


def touched_ssim(planes, H, W, same):
    Hm, Wm = (H, W) if same else (H - 10, W - 10)
    return ssim_tiles(Hm, Wm) * planes * 4


def touched_ssim_tiles(B, H, W, border, same):
    h, w = H - 2 * int(H * border), W - 2 * int(W * border)
    Hm, Wm = (h, w) if same else (h - 10, w - 10)
    nbs = ssim_tiles(Hm, Wm) * B
    return r16(nbs * 4) + nbs * 4           # the sums, rounded up to 16, then the counts


def menu_pair(seed, planes, H, W):
    from tests import loss_menu_ref as M
    if H >= 11 and W >= 11:
        p, g = M.dem_pair(seed, (planes, 1, H, W))
        return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(g[:, 0])
    return loss_pair(seed, planes, H, W)


def window_plane(seed, planes, H, W):
    """The plane of a "window" rule case: scattered voids, and the last plane's first 32 x 32 map tile left with nothing
    counted (a void every 11 pixels both ways puts one under every window there)."""
    v = void_plane(seed, (planes, H, W), holes=2)
    v[-1, 5:min(H, 48):11, 5:min(W, 48):11] = 0
    return v


def _keys(terms, with_base):
    slots = ([0, 1, 2] if with_base else []) + [3 + b for b in range(4) if terms & (1 << b)]
    ks = (ctypes.c_int * len(slots))(*slots)
    kw = (ctypes.c_double * len(slots))(*[1.0 + 0.25 * s for s in slots])
    sw = (ctypes.c_double * 7)(*[1.0 + 0.25 * s for s in range(7)])
    return slots, ks, kw, sw


def run_menu(ctx, terms, planes, H, W, alloc=None, masked=0, rule=1):
    """masked: 0 jspsr_loss_menu_*, 1 jspsr_loss_menu_valid_*, 2 jspsr_loss_menu_valid_ssim_*"""
    aP, aH, aW = alloc or (planes, H, W)
    p, g = menu_pair(61, aP, aH, aW)
    pp, gp = ctx.inp("pred", p), ctx.inp("gt", g)
    slots, ks, kw, sw = _keys(terms, True)
    base = ctx.inp("base_losses", np.array([0.125, 0.25, 0.5], np.float32))
    up = ctx.inp("grad_total", np.array([0.5], np.float32))
    out = ctx.out("out", (len(slots) + 1,), np.float32)
    gpred = ctx.acc("grad_pred", small_ints(62, (aP, aH, aW)))          # "the backward ... ADDS ... to grad_pred"
    ws = ctx.ws()
    if masked == 0:
        ctx.call("jspsr_loss_menu_forward", pp, gp, terms, planes, H, W, len(slots), ks, kw, base, out, ws, ctx.stream)
        ctx.call("jspsr_loss_menu_backward", pp, gp, terms, planes, H, W, sw, up, gpred, ws, ctx.stream)
        return
    v = window_plane(63, aP, aH, aW) if masked == 2 else void_plane(63, (aP, aH, aW))
    vp = ctx.inp("valid", v)
    if masked == 1:
        ctx.call("jspsr_loss_menu_valid_forward", pp, gp, vp, terms, planes, H, W, len(slots), ks, kw, base, out, ws, ctx.stream)
        ctx.call("jspsr_loss_menu_valid_backward", pp, gp, vp, terms, planes, H, W, sw, up, gpred, ws, ctx.stream)
    else:
        ctx.call("jspsr_loss_menu_valid_ssim_forward", pp, gp, vp, terms, planes, H, W, rule, len(slots), ks, kw, base, out, ws,
                 ctx.stream)
        ctx.call("jspsr_loss_menu_valid_ssim_backward", pp, gp, vp, terms, planes, H, W, rule, sw, up, gpred, ws, ctx.stream)


def menu_launches(terms, masked):
    v = "_valid" if masked else ""
    L = {f"loss_menu{v}_combine": 1}
    if terms & T_BERHU:
        L[f"loss_menu{v}_max"] = 1
    if terms & 7:
        L[f"loss_menu{v}_sum"] = 1
        L[f"loss_menu{v}_backward"] = 1
    if terms & T_SSIM:
        L["ssim_valid_forward" if masked else "ssim_forward"] = 1
        L["ssim_valid_backward" if masked else "ssim_backward"] = 1
    return L


def run_ssim(ctx, planes, H, W, same, alloc=None):
    aP, aH, aW = alloc or (planes, H, W)
    p, g = menu_pair(64, aP, aH, aW)
    out = ctx.out("out", (1,), np.float32)
    ctx.call("jspsr_ssim_forward", ctx.inp("pred", np.clip(p, 0, 1)), ctx.inp("gt", g), planes, H, W, same, None, out, ctx.ws(),
             ctx.stream)


def run_ssim_tiles(ctx, B, H, W, border, same, alloc=None, with_plane=True):
    aB, aH, aW = alloc or (B, H, W)
    p, g = menu_pair(65, aB, aH, aW)
    vp = ctx.inp("valid", window_plane(66, aB, aH, aW)) if with_plane else None
    out, counts = ctx.out("out", (aB,), np.float32), ctx.out("counts", (aB,), np.int32)
    ctx.call("jspsr_ssim_tiles_forward", ctx.inp("pred", p), ctx.inp("gt", g), vp, B, H, W, ctypes.c_double(border), same, None,
             out, counts, ctx.ws(), ctx.stream)


POINTWISE_SHAPES = [((1, 1, 1), "1 block; pmax 4 -> 16, psum 12 -> 16"), ((1, 1, 257), "2 blocks; pmax 8 -> 16, psum 24 -> 32"),
                    ((1, 3, 256), "3 blocks; psum 36 -> 48, counts 12 -> 16"), ((2, 8, 64), "4 blocks; no rounding"),
                    ((1, 300, 256), "max pass capped at 256 blocks, sum pass at 300"), ((1, 725, 725), "sum pass capped at 2048 blocks")]
SSIM_SHAPES = [((1, 11, 11), "one map element; ssum 4 -> 16, coef 12 -> 16"), ((2, 11, 40), "2 planes, 1 x 30 map; coef 720, no rounding"),
               ((6, 45, 70), "35 x 60 map: two tiles across, two down; ssum 96")]
MENU_CASES = [(7, s, w) for s, w in POINTWISE_SHAPES] + [(8, s, "SSIM alone: th never touched; " + w) for s, w in SSIM_SHAPES] + \
             [(15, s, "all four terms; " + w) for s, w in SSIM_SHAPES[1:]] + [(2, (1, 3, 256), "no BerHu: th and pmax never touched")]


# ---- one tile's meters (csrc/metrics.hip) ----------------------------------------------------------------------------------
SEL_STATE = 24      # struct SelState: uint32, (pad), uint64, float, float


def metric_blocks(n):
    return clamp(cdiv(n, 256 * 8), 1, 1024)


def touched_metrics(H, W):
    # the regions sit where the UNCROPPED raster puts them: dh (H W floats), the partial rows (2 floats per block of the
    # uncropped count), both rounded up to 16, the 256-bin histogram, three select states
    return r16(H * W * 4) + r16(metric_blocks(H * W) * 2 * 4) + 256 * 4 + 3 * SEL_STATE


def eval_pair(seed, H, W):
    """One tile in eval_ref's manner: a smooth [0,1] field and a noisy prediction that leaves [0,1] at a few pixels."""
    from tests import loss_menu_ref as M
    p, g = M.dem_pair(seed, (1, 1, max(H, 12), max(W, 12)))
    return np.ascontiguousarray(p[0, 0, :H, :W]), np.ascontiguousarray(g[0, 0, :H, :W])


def run_metrics(ctx, H, W, alloc=None, border=0.05):
    aH, aW = alloc or (H, W)
    p, g = eval_pair(21, aH, aW)
    pp, gp = ctx.inp("pred", p), ctx.inp("gt", g)
    scores = ctx.out("scores", (5,), np.float32)
    c_f = ctypes.c_float
    ctx.call("jspsr_metrics_forward", pp, gp, H, W, c_f(border), c_f(-10.0), c_f(2000.0), 0, scores, ctx.ws(), ctx.stream)


# metrics_forward counts its 24 select launches under one label, once
METRICS_LAUNCHES = {"metrics_prepare": 1, "metrics_reduce": 1, "metrics_select": 1}
METRICS_SHAPES = [((1, 1), "1 block; dh rounded 4 -> 16, rows 8 -> 16"), ((50, 100), "3 blocks; rows rounded 24 -> 32; cropped"),
                  ((64, 64), "2 blocks; no rounding"), ((1449, 1449), "block cap 1024; dh rounded + 12")]


# ---- a batch's meters (csrc/scores.hip) ------------------------------------------------------------------------------------
LDS_MAX_N = (163840 - 1664) // 8            # 20 272 pixels: above it the rasters are staged in the workspace


def touched_scores(masked, B, H, W, border=0.0):
    h, w = H - 2 * int(H * border), W - 2 * int(W * border)
    if h * w <= LDS_MAX_N:
        return 0                            # the path follows the CROP; one launch out of LDS addresses no workspace byte
    rows, rows_full = metric_blocks(h * w), metric_blocks(H * W)        # the grid of the crop; the layout of the raster
    plane = r16(B * H * W * 4)              # P and G, each laid out for the uncropped size
    off = 2 * plane + r16(B * rows_full * 4 * 8)        # partial: four doubles per (tile, block)
    off += B * 256 * 4                      # one histogram per tile
    end = off + B * 3 * 16                  # three select states of 16 bytes per tile
    if masked:
        end = off + r16(B * 3 * 16) + B * rows * 4 * 4 - 4              # {N, N_sl, N_sk, -} per (tile, block): the fourth unused
    return end


def run_scores(ctx, masked, B, H, W, border=0.0, alloc=None):
    aB, aH, aW = alloc or (B, H, W)
    p, g = menu_pair(71, aB, max(aH, 12), max(aW, 12))
    p, g = np.ascontiguousarray(p[:, :aH, :aW]), np.ascontiguousarray(g[:, :aH, :aW])
    pp, gp = ctx.inp("pred", p), ctx.inp("gt", g)
    scores = ctx.out("scores", (aB, 8), np.float32)
    c_f = ctypes.c_float
    tail = (c_f(border), c_f(-10.0), c_f(2000.0), 0, scores)
    if masked:
        counts = ctx.out("counts", (aB, 3), np.int32)
        ctx.call("jspsr_scores_batch_valid_forward", pp, gp, ctx.inp("valid", void_plane(72, (aB, aH, aW))), B, H, W, *tail, counts,
                 ctx.ws(), ctx.stream)
    else:
        ctx.call("jspsr_scores_batch_forward", pp, gp, B, H, W, *tail, ctx.ws(), ctx.stream)


def scores_launches(masked, H, W, border=0.0):
    h, w = H - 2 * int(H * border), W - 2 * int(W * border)
    name = "scores_batch_valid" if masked else "scores_batch"
    return {f"{name} (lds)": 1} if h * w <= LDS_MAX_N else {f"{name} (stream)": 27}


SCORES_CASES = [((1, 3, 3), 0.0, "LDS path, the smallest raster: 16 bytes, none touched"),
                ((5, 142, 142), 0.0, "LDS path at its largest raster, B = 5: none touched"),
                ((1, 143, 142), 0.0, "stream path, the smallest raster above 20 272; planes 81 224 -> 81 232"),
                ((5, 143, 142), 0.0, "stream path, B = 5; planes 406 120 -> 406 128"),
                ((2, 150, 160), 0.05, "stream layout, cropped to 136 x 144 = 19 584: the LDS launch, nothing touched"),
                ((2, 300, 200), 0.1, "stream path, cropped: 19 blocks in a layout of 30")]


# ---- propagation (csrc/prop.hip, prop_dma.hip, prop_head.hip, prop_head_dma.hip, prop_steps.hip) ---------------------------
NRED = 10                                   # grad_wk[9] + grad_b0: one row of 10 floats per workgroup
PROP_FORMS = [{"JSPSR_PROP_SPLIT": "0", "JSPSR_PROP_HEAD_SPLIT": "0"}, {"JSPSR_PROP_SPLIT": "1", "JSPSR_PROP_NW": "8"},
              {"JSPSR_PROP_NTL": "0", "JSPSR_PROP_WGS": "1", "JSPSR_PROP_HEAD_WGS": "1"},
              {"JSPSR_PROP_DMA": "0", "JSPSR_PROP_HEAD_DMA": "0"},
              {"JSPSR_PROP_SPLIT": "0", "JSPSR_PROP_RP": "2"}, {"JSPSR_PROP_SPLIT": "0", "JSPSR_PROP_RP": "4"}]      # test_prop_gpu's settings


def prop_takes_dma(entry, W, env):
    """Rows of 16-byte-aligned operands (the arenas') with W % 4 == 0 take the LDS-DMA kernels, unless switched off;
    fp32 heads never do."""
    if entry == "head_f32" or W % 4:
        return False
    return env.get("JSPSR_PROP_HEAD_DMA" if entry == "head_bf16" else "JSPSR_PROP_DMA", "1") != "0"


def prop_rows(entry, B, H, W, env=None):
    """Partial rows the backward of `entry` (planar, logits, head_f32, head_bf16) may write: its grid, or the grid's bound
    where the grid also depends on the chip's CU count."""
    env = env or {}
    if not prop_takes_dma(entry, W, env):
        return B * cdiv(W, 64) * cdiv(H, 8)                 # one workgroup per 8 x 64 tile
    rows_per_tile = 4                                       # a wave per row, four waves
    if entry == "planar":                                   # make_plan: the lab forms; the logits entry has none
        nw = 8 if env.get("JSPSR_PROP_NW") == "8" else 4
        split = env.get("JSPSR_PROP_SPLIT", "0") != "0"     # the backward's default is symmetric waves
        rp = int(env.get("JSPSR_PROP_RP", "1")) if nw == 4 and not split and env.get("JSPSR_PROP_RP") in ("2", "4") else 1
        rows_per_tile = nw * rp
    return min(B * cdiv(W, 64) * cdiv(H, rows_per_tile), 4096)         # persistent workgroups, capped at 4096


def touched_prop(entry, B, H, W, env=None):
    return 16 + prop_rows(entry, B, H, W, env) * NRED * 4  # "header (row count) + rows": 16 bytes, then the rows


def touched_step(B, H, W, gdem=True):
    nblk = B * cdiv(W, 64) * cdiv(H, 8)
    if not gdem:
        return nblk * NRED * 4
    return r16(nblk * NRED * 4) + nblk * 24 * 80 * 4        # one 24 x 80 window per tile behind the rows


def prop_case(B, H, W, oc=18):
    from tests.test_prop_gpu import _rand_case
    dem, weight, offset, w, b, gout = _rand_case(B, H, W, 1.0, seed=B + H + W)
    if oc == 16:
        offset = np.concatenate((offset[:, :8].numpy(), offset[:, 10:].numpy()), 1)
    f = lambda t: np.ascontiguousarray(np.asarray(t, dtype=np.float32))
    return f(dem), f(weight), f(offset), f(w), f(b), f(gout)


def bf16_bits(a):
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def run_prop(ctx, B, H, W, oc=18, fold=False, alloc=None):
    dem, weight, offset, w, b, gout = prop_case(*(alloc or (B, H, W)), oc=oc)
    ins = [ctx.inp(n, a) for n, a in (("grad_out", gout), ("dem", dem), ("weight", weight), ("offset", offset))]
    wk = ctx.inp("wk", w)
    gw, go = ctx.out("grad_weight", weight.shape, np.float32), ctx.out("grad_offset", offset.shape, np.float32)
    gwk, gb = ctx.out("grad_wk", (9,), np.float32), ctx.out("grad_b0", (1,), np.float32)     # "overwritten (not accumulated)"
    ws = ctx.ws()
    if fold:            # the producer alone (grad_wk = grad_b0 = NULL), then the fold on its own
        ctx.call("jspsr_prop_backward_f32", *ins, oc, wk, gw, go, None, None, ws, B, H, W, ctx.stream)
        ctx.call("jspsr_prop_backward_fold_f32", ws, B, H, W, gwk, gb, ctx.stream)
    else:
        ctx.call("jspsr_prop_backward_f32", *ins, oc, wk, gw, go, gwk, gb, ws, B, H, W, ctx.stream)


def run_logits(ctx, B, H, W, alloc=None):
    dem, weight, offset, w, b, gout = prop_case(*(alloc or (B, H, W)), oc=16)
    head = np.concatenate((np.log(weight / (1 - weight)), offset), 1)                       # (B, 25, H, W): logits, offsets
    ghead = ctx.out("grad_head", head.shape, np.float32)
    gwk, gb = ctx.out("grad_wk", (9,), np.float32), ctx.out("grad_b0", (1,), np.float32)
    ctx.call("jspsr_prop_logits_backward_f32", ctx.inp("grad_out", gout), ctx.inp("dem", dem), ctx.inp("head", head), ctx.inp("wk", w),
             ghead, gwk, gb, ctx.ws(), B, H, W, ctx.stream)


def run_head(ctx, dt, B, H, W, alloc=None):
    import torch
    from tests.test_prop_gpu import _head_case
    aB, aH, aW = alloc or (B, H, W)
    dem, head, _, _, w, b, gout = _head_case(aB, aH, aW, torch.float32, seed=aB + aH + aW)
    f = lambda t: np.ascontiguousarray(t.numpy(), dtype=np.float32)
    hd = bf16_bits(f(head)) if dt == BF16 else f(head)
    ghead = ctx.out("grad_head", hd.shape, hd.dtype)
    gwk, gb = ctx.out("grad_wk", (9,), np.float32), ctx.out("grad_b0", (1,), np.float32)
    ctx.call("jspsr_prop_head_backward", dt, ctx.inp("grad_out", f(gout)), ctx.inp("dem", f(dem)), ctx.inp("head", hd), ctx.inp("wk", f(w)),
             ghead, gwk, gb, ctx.ws(), B, H, W, ctx.stream)


def run_step(ctx, B, H, W, gdem=True, alloc=None):
    aB, aH, aW = alloc or (B, H, W)
    dem, weight, offset, w, b, gout = prop_case(aB, aH, aW, oc=18)
    offset = np.clip(offset, -5.0, 5.0)     # every tap within tile + halo: no global float atomic, so the same bits on every run
    ins = [ctx.inp(n, a) for n, a in (("grad_out", gout), ("dem", dem), ("weight", weight), ("offset", offset))]
    gw, go = ctx.out("grad_weight", weight.shape, np.float32), ctx.out("grad_offset", offset.shape, np.float32)    # accumulate = 0
    gd = ctx.acc("grad_dem", small_ints(91, dem.shape)) if gdem else None                    # "ADDED into it"
    gwk = ctx.out("grad_wk", (9,), np.float32) if gdem else None
    gb = ctx.out("grad_b0", (1,), np.float32) if gdem else None
    ctx.call("jspsr_prop_step_backward_f32", *ins, 18, ctx.inp("wk", w), ctypes.c_float(1.0), 1, 0, gw, go, gd, gwk, gb, ctx.ws(),
             B, H, W, ctx.stream)


def prop_launches(entry, W, env=None, fold=False):
    dma = " (dma)" if prop_takes_dma(entry, W, env or {}) else ""
    if entry == "planar":
        return {f"prop_backward{dma}": 1, ("prop_backward_fold" if fold else "prop_backward_finalize"): 1}
    if entry == "logits":
        return {f"prop_logits_backward{dma}": 1, "prop_backward_finalize": 1}
    return {f"prop_head_backward{dma}": 1, "prop_head_backward_finalize": 1}


# below one tile; ragged; a run crossing images; more general-path tiles than the 4096 rows the DMA grid is capped at
PROP_SHAPES = [((3, 8, 8), "below one tile"), ((1, 3, 64), "fewer rows than a tile"), ((2, 37, 53), "ragged, W % 4 != 0: general path"),
               ((2, 6, 132), "ragged, W = 2 tiles + 4"), ((5, 20, 72), "a run crossing images"),
               ((4097, 1, 3), "4097 general-path tiles: the max() takes nblk, not the 4096 floor")]


def prop_cases():
    """Every case of the three propagation queries (also what a child process of one switch setting runs)."""
    out = []
    for i, (s, why) in enumerate(PROP_SHAPES):
        oc = 16 if i % 2 else 18
        out.append((f"prop-{_x(s)}-oc{oc}", "jspsr_prop_backward_workspace_bytes", s, _bind(run_prop, *s, oc=oc), "planar", {}, why))
    for s in ((2, 37, 53), (5, 20, 72)):
        out.append((f"prop_fold-{_x(s)}", "jspsr_prop_backward_workspace_bytes", s, _bind(run_prop, *s, oc=16, fold=True), "planar",
                    {"fold": True}, "producer with grad_wk = NULL, then jspsr_prop_backward_fold_f32"))
    for s, why in (PROP_SHAPES[0], PROP_SHAPES[2], PROP_SHAPES[4], (PROP_SHAPES[5][0], "4097 tiles of the logits entry's 8 x 64 form")):
        out.append((f"prop_logits-{_x(s)}", "jspsr_prop_backward_workspace_bytes", s, _bind(run_logits, *s), "logits", {}, why))
    for dt, name in ((F32, "head_f32"), (BF16, "head_bf16")):
        for s, why in PROP_SHAPES if dt == BF16 else (PROP_SHAPES[0], PROP_SHAPES[2], PROP_SHAPES[5]):
            out.append((f"prop_{name}-{_x(s)}", "jspsr_prop_head_backward_workspace_bytes", s, _bind(run_head, dt, *s), name, {}, why))
    return out


# ---- weight gradient (csrc/wgrad.hip) ---------------------------------------------------------------------------------------
def wgrad_plan(dt, M, Cg, Ktot):
    """make_plan: split-K slices of the generic kernel."""
    bkm = 64 if dt == BF16 else 32
    bmc = 128 if Cg > 64 else (64 if Cg > 32 else 32)
    tiles = cdiv(Cg, bmc) * cdiv(Ktot, 128)
    splits = max(1, min(cdiv(768, tiles), cdiv(M, 4 * bkm)))
    per = cdiv(cdiv(M, splits), bkm) * bkm
    return cdiv(M, per)


def wgrad_patch_units(dt, B, H, W, Cg, Cx):
    """make_patch_plan: (strip, row block) units of the nine-tap kernel, or 0 where it does not apply."""
    U = 64 if dt == BF16 else 32
    if W % U or Cg < 32 or Cx < 32:
        return 0
    pairs, strips = cdiv(Cg, 64) * cdiv(Cx, 64), B * (W // U)
    want = max(1, cdiv(256, pairs * strips))
    rows = cdiv(H, want)
    if rows < 8:
        rows = min(H, 8)
    return strips * cdiv(H, rows)


def touched_wgrad(dt, B, OH, OW, Cg, Cx, KH, KW, nine_tap=False):
    slabs = wgrad_patch_units(dt, B, OH, OW, Cg, Cx) if nine_tap else wgrad_plan(dt, B * OH * OW, Cg, KH * KW * Cx)
    return slabs * Cg * KH * KW * Cx * 4    # one fp32 slab [Cg][KH KW Cx] per slice, whole


def run_wgrad(ctx, dt, B, OH, OW, Cg, Cx, KH, KW, stride=1, alloc_b=None):
    aB = alloc_b or B
    pad = KH // 2
    IH, IW = (OH - 1) * stride + KH - 2 * pad, (OW - 1) * stride + KW - 2 * pad
    if stride == 2:
        IH, IW = 2 * OH, 2 * OW
    rs = np.random.RandomState(95)
    g, x = rs.randint(-2, 3, (aB, OH, OW, Cg)).astype(np.float32), rs.randint(-2, 3, (aB, IH, IW, Cx)).astype(np.float32)
    if dt == BF16:
        g, x = bf16_bits(g), bf16_bits(x)
    dW = ctx.out("dW", (Cg, Cx, KH, KW), np.float32)            # accumulate = 0: written
    ctx.call("jspsr_conv2d_wgrad", dt, ctx.inp("G", g), Cg, Cg, 0, ctx.inp("X", x), Cx, Cx, 0, dW, Cg, Cx, B, OH, OW, IH, IW, KH, KW,
             stride, pad, 0, None, 0, ctx.ws(), ctx.stream)


# ---- the two BatchNorm backwards of a projecting block (csrc/elementwise.hip) -----------------------------------------------
def touched_bn_pair(dt, C, npix):
    from tests import perchannel_exact_ref as P
    chunks = P.make_red(npix, 1, C, 4 if dt == F32 else 8)["chunks"]
    return (6 * C + chunks * 3 * C) * 4     # "coef [6][C], then partial rows [chunks][3][C]"


def run_bn_pair(ctx, dt, C, npix, alloc_c=None):
    aC = alloc_c or C
    rs = np.random.RandomState(96)
    t = lambda: rs.randint(-3, 4, (npix, aC)).astype(np.float32)
    conv = (lambda a: bf16_bits(a)) if dt == BF16 else (lambda a: a)
    dy, x2, xd = conv(t()), conv(t()), conv(t())
    v = lambda lo, hi: rs.uniform(lo, hi, aC).astype(np.float32)
    mask_bytes = ctx.lib.jspsr_bn_mask_bytes(dt, npix, aC)
    mask = rs.randint(0, 256, max(mask_bytes, 1)).astype(np.uint8)
    par = [ctx.inp(n, a) for n, a in (("gamma2", v(0.5, 1.5)), ("mean2", v(-1, 1)), ("invstd2", v(0.5, 2)))]
    pard = [ctx.inp(n, a) for n, a in (("gammad", v(0.5, 1.5)), ("meand", v(-1, 1)), ("invstdd", v(0.5, 2)))]
    dx2, dxd = ctx.out("dx2", dy.shape, dy.dtype), ctx.out("dxd", dy.shape, dy.dtype)
    grads = [ctx.out(n, (aC,), np.float32) for n in ("dgamma2", "dbeta2", "dgammad", "dbetad")]     # accumulate = 0
    ctx.call("jspsr_bn_backward_pair", dt, ctx.inp("dy", dy), aC, 0, ctx.inp("mask", mask), ctx.inp("x2", x2), aC, 0, *par, 1,
             ctypes.c_float(0.5), ctx.inp("xd", xd), aC, 0, *pard, 1, dx2, dxd, grads[0], grads[1], 0, grads[2], grads[3], 0, npix, C,
             ctx.ws(), ctx.stream)


BN_PAIR_LAUNCHES = {"bn_bwd_reduce_pair": 1, "bn_bwd_finalize_pair": 1, "bn_bwd_apply_pair": 1}


# ---- the pooled family (csrc/summary.hip, csrc/strata.hip, csrc/errdist.hip) ----------------------------------------------
CHUNK, NSTATE, ROW_STATE, NOUT = 8192, 6, 64, 11


def hist_replicas(rows, chunks):
    r = 1
    while r < 16 and r * 64 < chunks and rows * 2 * r * NSTATE * 256 * 4 <= 64 << 20:
        r *= 2
    return r


def touched_summary(masked, n_cand, n_seg, total, chunks):
    rows = n_cand * n_seg
    off = r16(n_cand * total * 4)           # e: one float per (candidate, pooled element)
    off += r16(n_cand * chunks * 8)         # the chunk sums, fp64
    off += rows * hist_replicas(rows, chunks) * NSTATE * 256 * 4        # the histograms, cleared by the entry itself
    if masked:
        off += r16(chunks * 4)              # the chunk counts
    end = off + rows * ROW_STATE
    if masked:
        end += 64 + total                   # one keep byte per pooled element, 64 bytes behind the row states
    return end


def touched_strata(n_cand, n_classes, total):
    rows, runs = n_cand * n_classes, cdiv(total, CHUNK)
    off = r16(n_cand * total * 4) + r16(n_cand * runs * n_classes * 8) + rows * hist_replicas(rows, runs) * NSTATE * 256 * 4
    return off + rows * ROW_STATE + 64 + total          # the class bytes sit 64 bytes behind the row states


def touched_errdist(n_cand, gridsize):
    return (n_cand - 1) * 8 * 8 + 16        # {n, bw} at the head of each candidate's row of 8 doubles


# name -> (n_cand, n_segments, windows (segment, h, w) cut out of a (H, W) raster with pitch W)
POOLS = {"one": (1, 1, [(0, 5, 7)]),                                             # 35 elements: one chunk
         "ragged": (3, 2, [(0, 90, 100), (0, 30, 41), (1, 3, 5)]),               # 10 230 + 15: chunks 2 + 1, both last ones ragged
         "replicas": (1, 1, [(0, 730, 730)])}                                    # 66 chunks: two histogram replicas


def pool_sizes(tag):
    n_cand, n_seg, wins = POOLS[tag]
    seg_n = [sum(h * w for sg, h, w in wins if sg == k) for k in range(n_seg)]
    return n_cand, n_seg, sum(seg_n), sum(cdiv(n, CHUNK) for n in seg_n)


def pool_operands(ctx, tag, masked):
    """The rasters and the window table of a pool -> what every pooled entry takes first."""
    from jspsr_amd import summary as S
    n_cand, n_seg, wins = POOLS[tag]
    H, W = max(h for _, h, w in wins) + 3, sum(w for _, h, w in wins) + 2 * len(wins)
    rs = np.random.RandomState(81)
    gt = (100.0 + 10.0 * rs.standard_normal((H, W))).astype(np.float32)
    cands = [(gt + (0.5 + 0.25 * c) * rs.standard_normal((H, W))).astype(np.float32) for c in range(n_cand)]
    windows, x0 = [], 1
    for sg, h, w in wins:                   # side by side, one row down, pitch W: crops read in place
        at = (W + x0, W)
        windows.append((sg, h, w, at, [at] * n_cand))
        x0 += w + 2
    cp = (ctypes.c_void_p * n_cand)(*[ctx.inp(f"cand{c}", a) for c, a in enumerate(cands)])
    cn = (ctypes.c_longlong * n_cand)(*[H * W] * n_cand)
    valid = void_plane(82, (1, H, W))[0] if masked else None
    return S, cp, cn, n_cand, ctx.inp("gt", gt), H * W, valid, windows, (H, W)


def run_summary(ctx, masked, tag):
    S, cp, cn, n_cand, gp, gn, valid, windows, _ = pool_operands(ctx, tag, masked)
    _, n_seg, total, chunks = pool_sizes(tag)
    seg, start, chunk = np.zeros((n_seg, S._SEG_WORDS), np.int64), 0, 0
    for k in range(n_seg):
        n = sum(h * w for sg, h, w, _, _ in windows if sg == k)
        m0, m1, l0, l1, g = S.segment_ranks(n)
        seg[k] = (start, n, chunk, m0, m1, l0, l1, np.float64(g).view(np.int64))
        start, chunk = start + n, chunk + cdiv(n, CHUNK)
    wp, sp = ctx.inp("windows", S._window_table(windows, True)), ctx.inp("segments", seg)
    out = ctx.out("out", (n_cand, n_seg, NOUT), np.float32)
    tail = (wp, len(windows), sp, n_seg, total, chunks, ctypes.c_double(100.0), out)
    if masked:
        counts = ctx.out("counts", (n_seg,), np.int64)
        ctx.call("jspsr_summary_valid_forward", cp, cn, n_cand, gp, gn, ctx.inp("valid", valid), gn, *tail, counts, ctx.ws(), ctx.stream)
    else:
        ctx.call("jspsr_summary_forward", cp, cn, n_cand, gp, gn, *tail, ctx.ws(), ctx.stream)


def run_strata(ctx, tag, n_classes, with_plane):
    S, cp, cn, n_cand, gp, gn, valid, windows, (H, W) = pool_operands(ctx, tag, with_plane)
    total = pool_sizes(tag)[2]
    labels = np.random.RandomState(83).randint(0, n_classes + 1, (H, W)).astype(np.uint8)      # n_classes: a label of no class
    labels[0, :] = 255
    out, counts = ctx.out("out", (n_cand, n_classes, NOUT), np.float32), ctx.out("counts", (n_classes,), np.int64)
    ctx.call("jspsr_strata_forward", cp, cn, n_cand, gp, gn, ctx.inp("labels", labels), gn, n_classes,
             ctx.inp("valid", valid) if with_plane else None, gn if with_plane else 0, ctx.inp("windows", S._window_table(windows, False)),
             len(windows), total, ctypes.c_double(100.0), out, counts, ctx.ws(), ctx.stream)


def run_errdist(ctx, n_cand, gridsize, alloc=None):
    key0, K = ctypes.c_int(), ctypes.c_int()
    assert ctx.lib.jspsr_errdist_bins(-5.0, 5.0, ctypes.byref(key0), ctypes.byref(K)) == 0
    key0, K = key0.value, K.value
    a_cand, a_grid = alloc or (n_cand, gridsize)
    hist = np.random.RandomState(84).poisson(0.3, (a_cand, K)).astype(np.int64)
    if a_grid > 1000:
        hist[:, 64:] = 0                    # a long grid: few occupied bins keep the density pass short
    hist[-1] = 0                            # the last candidate has no element: NaN curve, by the kernels' own branch
    if a_cand > 1:
        hist[0] = 0
        hist[0, K // 2] = 1                 # one element: no variance
    support, density = ctx.out("support", (a_cand, a_grid), np.float64), ctx.out("density", (a_cand, a_grid), np.float64)
    stats = ctx.out("stats", (a_cand, 3), np.float64)
    ctx.call("jspsr_errdist_kde_forward", ctx.inp("hist", hist), n_cand, key0, K, gridsize, ctypes.c_double(0.5), ctypes.c_double(1.0),
             support, density, stats, ctx.ws(), ctx.stream)


# ---- optimizer ranges (csrc/optim.hip) -------------------------------------------------------------------------------------
def optim_blocks(n):
    return clamp(cdiv(n // 4, 256), 1, 4096)


def touched_optim(n):
    return optim_blocks(n) * 16 - 4         # rows of {min, max, bad, -}: the fourth float of a row is never addressed


def touched_ranges(count):
    return count * 64 * 16 - 4              # grid (64, count), rows as above


def run_optim(ctx, n, kind=2):
    rs = np.random.RandomState(31)
    g = rs.standard_normal(n).astype(np.float32)
    if n > 8:
        g[5] = np.inf
    p = ctx.acc("param", rs.standard_normal(n).astype(np.float32))
    m = ctx.acc("exp_avg", np.zeros(n, np.float32))
    v = ctx.acc("exp_avg_sq", np.zeros(n, np.float32))
    rng = ctx.acc("grad_range", np.array([999.0, -999.0, 0.0, 0.0], np.float32))      # "FOLDS the result into grad_range"
    c_f = ctypes.c_float
    ctx.call("jspsr_optim_step", kind, p, ctx.inp("grad", g), m, v, n, c_f(1e-3), c_f(0.9), c_f(0.999), c_f(1e-8), c_f(1e-6),
             1, None, rng, ctx.ws(), ctx.stream)


def run_ranges(ctx, count):
    rs = np.random.RandomState(32)
    sizes = [1, 255, 64 * 256 + 3, 7, 1000, 3, 16385, 2][:count]
    ptrs, dts = [], []
    for k, n in enumerate(sizes):
        if k % 2:
            x = (rs.standard_normal(n).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)      # bf16 bits
            dts.append(BF16)
        else:
            x = rs.standard_normal(n).astype(np.float32)
            dts.append(F32)
        ptrs.append(ctx.inp(f"t{k}", x))
    tp = (ctypes.c_void_p * count)(*ptrs)
    nn = (ctypes.c_longlong * count)(*sizes)
    dd = (ctypes.c_int * count)(*dts)
    table = ctx.out("table", (count, 4), np.float32)              # "table[k][4] receives {min, max, count, 0}"
    ctx.call("jspsr_tensor_ranges", count, tp, nn, dd, table, ctx.ws(), ctx.stream)


# ---- gate MLP backward (csrc/elementwise.hip) ------------------------------------------------------------------------------
def touched_gate(B, C, Ch):
    return (B * C + B * 2 * Ch) * 4         # dz (B, C) then dh (B, 2, Ch), fp32, back to back


def run_gate(ctx, B, C, Ch, alloc=None):
    aB, aC, aCh = alloc or (B, C, Ch)
    rs = np.random.RandomState(41)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    ds, hid, avg, mx = f(aB, aC), f(aB, 2, aCh), f(aB, aC), f(aB, aC)
    s = (1.0 / (1.0 + np.exp(-f(aB, aC)))).astype(np.float32)
    w1, w2 = f(aCh, aC) * 0.1, f(aC, aCh) * 0.1
    ins = [ctx.inp(n, a) for n, a in (("ds", ds), ("s", s), ("hid", hid), ("avg", avg), ("mx", mx), ("w1", w1), ("w2", w2))]
    outs = [ctx.out("davg", (aB, aC), np.float32), ctx.out("dmax", (aB, aC), np.float32),
            ctx.out("dw1", (aCh, aC), np.float32), ctx.out("dw2", (aC, aCh), np.float32)]
    ctx.call("jspsr_gate_mlp_backward", *ins, B, C, Ch, *outs, ctx.ws(), ctx.stream)


GATE_LAUNCHES = {"gate_mlp_bwd_hidden": 1, "gate_mlp_bwd_in": 1, "gate_mlp_wgrad": 1}


# ---- nearest seed (csrc/scene_voids.hip) -----------------------------------------------------------------------------------
def scenes_of(tag):
    """(offset, H, W) rows, back to back, covering the whole plane."""
    shapes = {"column": [(5, 1)], "bands": [(65, 3)], "three": [(3, 7), (70, 2), (1, 1)]}[tag]
    rows, off = [], 0
    for h, w in shapes:
        rows.append((off, h, w))
        off += h * w
    return rows, off


def touched_seed(pixels):
    return 2 * pixels                       # "2 B per pixel": one int16 per pixel of every scene, the scenes cover the plane


def run_seed(ctx, tag):
    rows, pixels = scenes_of(tag)
    rs = np.random.RandomState(51)
    seed = (rs.uniform(size=pixels) < 0.2).astype(np.uint8)
    table = np.array(rows, np.int64)
    host = (ctypes.c_longlong * table.size)(*table.flatten().tolist())
    src, d2 = ctx.out("src", (pixels,), np.int32), ctx.out("d2", (pixels,), np.int32)
    ctx.call("jspsr_scene_nearest_seed", ctx.inp("seed", seed), pixels, ctx.inp("scenes", table), host, len(rows), 0, src, d2,
             ctx.ws(), ctx.stream)


# ---- the table -------------------------------------------------------------------------------------------------------------
def _bind(fn, *a, **k):
    return lambda ctx: fn(ctx, *a, **k)


CASES = []
for _s, _why in LOSS_SHAPES:
    CASES.append(Case(f"loss-{_s[0]}x{_s[1]}x{_s[2]}", "jspsr_loss_workspace_bytes", _s, _bind(run_loss, *_s), LOSS_LAUNCHES,
                      touched_loss, _why))
    CASES.append(Case(f"loss_valid-{_s[0]}x{_s[1]}x{_s[2]}", "jspsr_loss_valid_workspace_bytes", _s, _bind(run_loss_valid, *_s),
                      LOSS_VALID_LAUNCHES, touched_loss_valid, _why))
def _x(s):
    return "x".join(str(v) for v in s)


# loss_terms.hip: "Every reduction writes per-workgroup partials folded in a fixed order in double: the same bits on every
# run"; no atomics.  The header names no alignment for these workspaces: the 64-bit counts N and N_s need 8, the entries
# now ask for 16 (JSPSR_EALIGN) as the other families do.
for _t, _s, _why in MENU_CASES:
    CASES.append(Case(f"menu-t{_t}-{_x(_s)}", "jspsr_loss_menu_workspace_bytes", (_t,) + _s, _bind(run_menu, _t, *_s),
                      menu_launches(_t, 0), touched_menu, _why))
for _t, _s, _why in [(7, s, w) for s, w in POINTWISE_SHAPES] + [(6, (1, 3, 256), "no BerHu: th and pmax never touched")]:
    CASES.append(Case(f"menu_valid-t{_t}-{_x(_s)}", "jspsr_loss_menu_valid_workspace_bytes", (_t,) + _s,
                      _bind(run_menu, _t, *_s, masked=1), menu_launches(_t, 1), touched_menu_valid, _why))
for _t, _s, _why in [(8, s, w) for s, w in SSIM_SHAPES] + [(15, s, "all four terms; " + w) for s, w in SSIM_SHAPES[1:]] + \
                    [(7, (1, 3, 256), "no SSIM bit: the K19 layout alone")]:
    CASES.append(Case(f"menu_valid_ssim-t{_t}-{_x(_s)}", "jspsr_loss_menu_valid_ssim_workspace_bytes", (_t,) + _s + (1,),
                      _bind(run_menu, _t, *_s, masked=2), menu_launches(_t, 2), touched_menu_valid_ssim,
                      _why + "; window rule, a tile with nothing counted"))
SSIM_LAUNCHES = {"ssim_forward": 1, "ssim_finalize": 1}
for _s, _same, _why in [(s, 0, w.split(";")[0]) for s, w in SSIM_SHAPES] + [((1, 10, 10), 1, "same mode below 11: 1 tile; 4 -> 16"),
                                                                            ((3, 33, 40), 1, "same mode: 2 x 2 tiles, 3 planes; 48")]:
    CASES.append(Case(f"ssim-{_x(_s)}-same{_same}", "jspsr_ssim_workspace_bytes", _s + (_same,), _bind(run_ssim, *_s, _same),
                      SSIM_LAUNCHES, touched_ssim, _why))
TILES_LAUNCHES = {"ssim_tiles_forward": 1, "ssim_tiles_finalize": 1}
for _a, _kw, _why in [((1, 11, 11, 0.0, 0), {}, "B = 1, one map element; each half 4 -> 16"),
                      ((5, 45, 70, 0.05, 0), {}, "B = 5, cropped to 41 x 64: 1 x 2 tiles; each half 40 -> 48"),
                      ((2, 10, 10, 0.0, 1), {}, "same mode below 11, a plane"),
                      ((3, 33, 40, 0.0, 1), {"with_plane": False}, "same mode, valid = NULL; each half 48")]:
    CASES.append(Case(f"ssim_tiles-{_x(_a)}", "jspsr_ssim_tiles_workspace_bytes", _a, _bind(run_ssim_tiles, *_a, **_kw),
                      TILES_LAUNCHES, touched_ssim_tiles, _why))
# prop: rows written once per workgroup, folded in double in a fixed order; a persistent workgroup's tiles are fixed by the
# grid: the same bits on every run of one chip
for _n, _q, _s, _run, _entry, _kw, _why in prop_cases():
    CASES.append(Case(_n, _q, _s, _run, prop_launches(_entry, _s[2], None, **_kw),
                      (lambda e: (lambda B, H, W: touched_prop(e, B, H, W)))(_entry), _why))
for _s, _why in PROP_SHAPES[:5]:
    CASES.append(Case(f"prop_step-{_x(_s)}", "jspsr_prop_step_backward_workspace_bytes", _s, _bind(run_step, *_s),
                      {"prop_step_backward": 1, "prop_step_gdem_gather": 1, "prop_step_backward_finalize": 1}, touched_step,
                      _why + "; rows and windows"))
CASES.append(Case("prop_step-2x37x53-rows_only", "jspsr_prop_step_backward_workspace_bytes", (2, 37, 53), _bind(run_step, 2, 37, 53, gdem=False),
                  {"prop_step_backward": 1}, lambda B, H, W: touched_step(B, H, W, False), "grad_dem = grad_wk = NULL: the rows alone"))
# wgrad: "split-K slabs, summed in a fixed order".  (dtype, B, OH, OW, Cg, Cx, KH, KW), stride, nine-tap?
WGRAD_CASES = [((F32, 1, 5, 5, 8, 12, 1, 1), 1, False, "generic plan, one slice"),
               ((F32, 2, 16, 17, 36, 132, 1, 1), 1, False, "generic plan, split-K = 5"),
               ((BF16, 2, 16, 16, 8, 16, 3, 3), 2, False, "generic plan (stride 2), split-K = 2, bf16"),
               ((BF16, 1, 5, 5, 8, 16, 1, 1), 1, False, "generic plan, one slice, bf16"),
               ((F32, 1, 9, 32, 32, 32, 3, 3), 1, True, "nine-tap plan: 2 units, fewer than the 3 generic slices the query counts"),
               ((BF16, 1, 9, 64, 32, 32, 3, 3), 1, True, "nine-tap plan, bf16: 2 units"),
               ((F32, 4, 16, 64, 512, 512, 3, 3), 1, True, "nine-tap plan: 8 units, more than the 6 generic slices: the max() takes them")]
for _a, _st, _nt, _why in WGRAD_CASES:
    CASES.append(Case(f"wgrad-{_x(_a)}-s{_st}", "jspsr_conv2d_wgrad_workspace_bytes", _a, _bind(run_wgrad, *_a, stride=_st),
                      {("conv2d_wgrad_patch" if _nt else "conv2d_wgrad"): 1, "conv2d_wgrad_reduce": 1},
                      (lambda nt: (lambda *a: touched_wgrad(*a, nine_tap=nt)))(_nt), _why))
for _dt, _c, _n, _why in [(F32, 8, 1, "one pixel, one chunk"), (BF16, 64, 2500, "40 chunks of 63 pixels, bf16"),
                          (F32, 1792, 300, "7 channel blocks: the query's 256-row floor is the larger term")]:
    # the query takes no pixel count: it sizes for the most chunks any count can get
    CASES.append(Case(f"bn_pair-{'bf16' if _dt else 'f32'}-c{_c}-n{_n}", "jspsr_bn_backward_pair_workspace_bytes", (_dt, _c),
                      _bind(run_bn_pair, _dt, _c, _n), BN_PAIR_LAUNCHES, (lambda n: (lambda dt, C: touched_bn_pair(dt, C, n)))(_n), _why))
for _m in (0, 1):
    for _s, _b, _why in SCORES_CASES:
        # bits: integer atomics only (histogram, counts); "the same bits ... on every run"
        _q = "jspsr_scores_batch_valid_workspace_bytes" if _m else "jspsr_scores_batch_workspace_bytes"
        CASES.append(Case(f"scores{'_valid' if _m else ''}-{_x(_s)}-b{_b}", _q, _s, _bind(run_scores, _m, *_s, border=_b),
                          scores_launches(_m, _s[1], _s[2], _b),
                          (lambda m, b: (lambda B, H, W: touched_scores(m, B, H, W, b)))(_m, _b), _why))
POOL_WHY = {"one": "1 candidate, 1 segment, 1 chunk; e 140 -> 144, sums 8 -> 16",
            "ragged": "3 candidates, 2 segments, ragged last chunks; e 122 940 -> 122 944, sums 72 -> 80, counts 12 -> 16, keep 10 245",
            "replicas": "66 chunks: 2 histogram replicas; counts 264 -> 272"}
for _m in (0, 1):
    for _t in POOLS:
        # bits: integer atomics only; the sums fold chunk by chunk in a fixed order ("the same bits on every run").  The
        # histograms and chunk counts are cleared by the entry's own hipMemsetAsync, not by the caller.
        CASES.append(Case(f"summary{'_valid' if _m else ''}-{_t}", f"jspsr_summary{'_valid' if _m else ''}_workspace_bytes",
                          pool_sizes(_t), _bind(run_summary, _m, _t),
                          {f"summary{'_valid' if _m else ''}_prepare": 1, f"summary{'_valid' if _m else ''}_select": 15},
                          (lambda m: (lambda *a: touched_summary(m, *a)))(_m), POOL_WHY[_t]))
for _t, _k, _v in [("one", 1, False), ("ragged", 3, True), ("replicas", 32, False), ("ragged", 32, False)]:
    _nc, _, _tot, _ = pool_sizes(_t)
    CASES.append(Case(f"strata-{_t}-k{_k}", "jspsr_strata_workspace_bytes", (_nc, _k, _tot), _bind(run_strata, _t, _k, _v),
                      {"strata_prepare": 1, "strata_select": 15}, touched_strata,
                      POOL_WHY[_t].split(";")[0] + f"; {_k} classes" + ("; 96 rows" if (_t, _k) == ("ragged", 32) else "")))
for _c, _g, _why in [(1, 2, "1 candidate, the smallest grid"), (3, 200, "3 candidates: an empty one and one without variance")]:
    # the query is n_cand rows of 8 doubles; fp64 tree sums in a fixed order
    CASES.append(Case(f"errdist-{_c}x{_g}", "jspsr_errdist_workspace_bytes", (_c, _g), _bind(run_errdist, _c, _g),
                      {"errdist_kde": 2}, touched_errdist, _why))
for _s, _why in METRICS_SHAPES:
    # bits: the histogram's integer atomics commute; the sums fold in a fixed order
    CASES.append(Case(f"metrics-{_s[0]}x{_s[1]}", "jspsr_metrics_workspace_bytes", _s, _bind(run_metrics, *_s), METRICS_LAUNCHES,
                      touched_metrics, _why))
for _n, _why in [(1, "1 row"), (3 * 1024 - 1, "3 rows, ragged tail"), (4096 * 1024 + 1027, "row cap 4096")]:
    # the query takes no argument: its one term is the row cap; min / max / a count below 2^24 do not depend on the order
    CASES.append(Case(f"optim-{_n}", "jspsr_optim_workspace_bytes", (), _bind(run_optim, _n),
                      {"optim_step": 1, "optim_step (range)": 1}, (lambda n: (lambda: touched_optim(n)))(_n), _why, align=4))
for _c, _why in [(1, "1 tensor"), (8, "8 tensors, the most")]:
    CASES.append(Case(f"ranges-{_c}", "jspsr_tensor_ranges_workspace_bytes", (), _bind(run_ranges, _c),
                      {"tensor_ranges": 1, "tensor_ranges (finalize)": 1}, (lambda c: (lambda: touched_ranges(c)))(_c), _why, align=4))
for _s, _why in [((1, 64, 4), "B = 1, C = 64"), ((2, 16128, 128), "(C + 2 Ch) * 4 = 64 KiB exactly"), ((3, 70, 5), "odd sizes")]:
    # every access is one fp32: 4-byte alignment is the contract (the header names none)
    CASES.append(Case(f"gate-{_s[0]}x{_s[1]}x{_s[2]}", "jspsr_gate_mlp_backward_workspace_bytes", _s, _bind(run_gate, *_s),
                      GATE_LAUNCHES, touched_gate, _why, align=4))
for _t, _why in [("column", "one column; 10 bytes rounded to 16"), ("bands", "65 rows: two bands; 390 rounded to 400"),
                 ("three", "three scenes; 324 rounded to 336")]:
    # integer arithmetic only; one label for the call's three launches
    CASES.append(Case(f"seed-{_t}", "jspsr_scene_nearest_seed_workspace_bytes", (scenes_of(_t)[1],), _bind(run_seed, _t),
                      {"scene_nearest_seed": 1}, touched_seed, _why, align=2))

REFUSALS = [
    Refusal("loss B=0", "jspsr_loss_workspace_bytes", (0, 8, 8), (1, 8, 8), lambda ctx, q, a: run_loss(ctx, *q, alloc=a),
            launches=LOSS_LAUNCHES),
    Refusal("loss_valid W=0", "jspsr_loss_valid_workspace_bytes", (1, 8, 0), (1, 8, 1),
            lambda ctx, q, a: run_loss_valid(ctx, *q, alloc=a), launches=LOSS_VALID_LAUNCHES),
    Refusal("metrics H=0", "jspsr_metrics_workspace_bytes", (0, 16), (1, 16), lambda ctx, q, a: run_metrics(ctx, *q, alloc=a, border=0.0),
            launches=METRICS_LAUNCHES),
    Refusal("gate above 64 KiB", "jspsr_gate_mlp_backward_workspace_bytes", (1, 16129, 128), (1, 16128, 128),
            lambda ctx, q, a: run_gate(ctx, *q, alloc=(1, 16129, 128)), launches=GATE_LAUNCHES),
    Refusal("menu SSIM H=10", "jspsr_loss_menu_workspace_bytes", (8, 1, 10, 12), (8, 1, 11, 12),
            lambda ctx, q, a: run_menu(ctx, *q, alloc=a[1:]), launches=menu_launches(8, 0)),
    Refusal("menu SSIM W=10", "jspsr_loss_menu_workspace_bytes", (15, 1, 12, 10), (15, 1, 12, 11),
            lambda ctx, q, a: run_menu(ctx, *q, alloc=a[1:]), launches=menu_launches(15, 0)),
    Refusal("menu terms=16", "jspsr_loss_menu_workspace_bytes", (16, 1, 12, 12), (4, 1, 12, 12),
            lambda ctx, q, a: run_menu(ctx, *q, alloc=a[1:]), launches=menu_launches(4, 0)),
    Refusal("menu planes=0", "jspsr_loss_menu_workspace_bytes", (7, 0, 12, 12), (7, 1, 12, 12),
            lambda ctx, q, a: run_menu(ctx, *q, alloc=a[1:]), launches=menu_launches(7, 0)),
    Refusal("menu_valid SSIM bit (not built)", "jspsr_loss_menu_valid_workspace_bytes", (15, 1, 12, 12), (7, 1, 12, 12),
            lambda ctx, q, a: run_menu(ctx, *q, alloc=a[1:], masked=1), launches=menu_launches(7, 1)),
    Refusal("menu_valid_ssim H=10", "jspsr_loss_menu_valid_ssim_workspace_bytes", (8, 1, 10, 12, 1), (8, 1, 11, 12, 1),
            lambda ctx, q, a: run_menu(ctx, *q[:4], alloc=a[1:4], masked=2, rule=q[4]), launches=menu_launches(8, 2)),
    Refusal("menu_valid_ssim rule=0", "jspsr_loss_menu_valid_ssim_workspace_bytes", (15, 1, 12, 12, 0), (15, 1, 12, 12, 1),
            lambda ctx, q, a: run_menu(ctx, *q[:4], alloc=a[1:4], masked=2, rule=q[4]), launches=menu_launches(15, 2)),
    Refusal("ssim H=10 valid mode", "jspsr_ssim_workspace_bytes", (1, 10, 12, 0), (1, 11, 12, 0),
            lambda ctx, q, a: run_ssim(ctx, *q, alloc=a[:3]), launches=SSIM_LAUNCHES),
    Refusal("ssim planes=65536", "jspsr_ssim_workspace_bytes", (65536, 1, 1, 1), (65535, 1, 1, 1),
            lambda ctx, q, a: run_ssim(ctx, *q, alloc=(65536, 1, 1)), launches=SSIM_LAUNCHES),
    Refusal("ssim_tiles B=0", "jspsr_ssim_tiles_workspace_bytes", (0, 12, 12, 0.0, 0), (1, 12, 12, 0.0, 0),
            lambda ctx, q, a: run_ssim_tiles(ctx, *q, alloc=a[:3]), launches=TILES_LAUNCHES),
    Refusal("ssim_tiles crop leaves 10 rows", "jspsr_ssim_tiles_workspace_bytes", (1, 12, 14, 0.1, 0), (1, 12, 14, 0.08, 0),
            lambda ctx, q, a: run_ssim_tiles(ctx, *q, alloc=a[:3]), launches=TILES_LAUNCHES),
    Refusal("scores H=2", "jspsr_scores_batch_workspace_bytes", (1, 2, 8), (1, 3, 8),
            lambda ctx, q, a: run_scores(ctx, 0, *q, alloc=a), launches=scores_launches(0, 3, 8)),
    Refusal("scores_valid W=2", "jspsr_scores_batch_valid_workspace_bytes", (2, 8, 2), (2, 8, 3),
            lambda ctx, q, a: run_scores(ctx, 1, *q, alloc=a), launches=scores_launches(1, 8, 3)),
    Refusal("scores B=0", "jspsr_scores_batch_workspace_bytes", (0, 8, 8), (1, 8, 8),
            lambda ctx, q, a: run_scores(ctx, 0, *q, alloc=a), launches=scores_launches(0, 8, 8)),
    Refusal("errdist gridsize=1", "jspsr_errdist_workspace_bytes", (1, 1), (1, 2),
            lambda ctx, q, a: run_errdist(ctx, *q, alloc=a), launches={"errdist_kde": 2}),
    Refusal("errdist gridsize=65536", "jspsr_errdist_workspace_bytes", (2, 65536), (2, 65535),
            lambda ctx, q, a: run_errdist(ctx, *q, alloc=(2, 65536)), launches={"errdist_kde": 2}),
    Refusal("errdist n_cand=9", "jspsr_errdist_workspace_bytes", (9, 8), (8, 8),
            lambda ctx, q, a: run_errdist(ctx, *q, alloc=(9, 8)), launches={"errdist_kde": 2}),
    Refusal("prop B=0", "jspsr_prop_backward_workspace_bytes", (0, 8, 8), (1, 8, 8),
            lambda ctx, q, a: run_prop(ctx, *q, alloc=a), launches=prop_launches("planar", 8)),
    Refusal("prop_logits H=0", "jspsr_prop_backward_workspace_bytes", (1, 0, 8), (1, 1, 8),
            lambda ctx, q, a: run_logits(ctx, *q, alloc=a), launches=prop_launches("logits", 8)),
    Refusal("prop_head W=0", "jspsr_prop_head_backward_workspace_bytes", (2, 8, 0), (2, 8, 1),
            lambda ctx, q, a: run_head(ctx, BF16, *q, alloc=a), launches=prop_launches("head_bf16", 1)),
    Refusal("prop_step B=0", "jspsr_prop_step_backward_workspace_bytes", (0, 8, 8), (1, 8, 8),
            lambda ctx, q, a: run_step(ctx, *q, alloc=a),
            launches={"prop_step_backward": 1, "prop_step_gdem_gather": 1, "prop_step_backward_finalize": 1}),
    Refusal("wgrad B=0", "jspsr_conv2d_wgrad_workspace_bytes", (F32, 0, 5, 5, 8, 12, 1, 1), (F32, 1, 5, 5, 8, 12, 1, 1),
            lambda ctx, q, a: run_wgrad(ctx, *q, alloc_b=1), launches={"conv2d_wgrad": 1, "conv2d_wgrad_reduce": 1}),
    Refusal("bn_pair C=0", "jspsr_bn_backward_pair_workspace_bytes", (F32, 0), (F32, 4),
            lambda ctx, q, a: run_bn_pair(ctx, q[0], q[1], 10, alloc_c=4), launches=BN_PAIR_LAUNCHES),
    Refusal("gate B=0", "jspsr_gate_mlp_backward_workspace_bytes", (0, 64, 4), (1, 64, 4), lambda ctx, q, a: run_gate(ctx, *q, alloc=a),
            launches=GATE_LAUNCHES),
]

# every census label a case or a refusal can produce: "unchanged census" means none of these moved
ALL_LAUNCHES = sorted({n for c in CASES for n in c.launches} | {n for r in REFUSALS for n in r.launches})

HELD = sorted({c.query for c in CASES})
ELSEWHERE = {
    "jspsr_head_backward_workspace_bytes": "tests/test_heads_exact_gpu.py::test_workspace_contracts",
    "jspsr_conv_head1_workspace_bytes": "tests/test_heads_exact_gpu.py::test_workspace_contracts",
    "jspsr_reduce_workspace_bytes": "tests/test_perchannel_exact_gpu.py",
}

# per query: arguments far above the test shapes, for touched <= query in exact integers (a 32-bit wrap inside a query
# shows here): the workload's 8 x 512 x 512, 64 x 1024 x 1024, and the largest raster the header admits
LARGE = {
    "jspsr_loss_workspace_bytes": [(8, 512, 512), (64, 1024, 1024), (1, 46340, 46340), (2147483647, 1, 1)],
    "jspsr_loss_valid_workspace_bytes": [(8, 512, 512), (64, 1024, 1024), (1, 46340, 46340), (2147483647, 1, 1)],
    "jspsr_metrics_workspace_bytes": [(512, 512), (1024, 1024), (46340, 46340), (2147483647, 1)],
    "jspsr_gate_mlp_backward_workspace_bytes": [(8, 512, 32), (64, 16128, 128), (2147483647, 1, 1), (65536, 8192, 4096)],
    "jspsr_scene_nearest_seed_workspace_bytes": [(8 * 512 * 512,), (64 * 1024 * 1024,), (16384 * 16384,), (32767 * 32767 * 4,)],
}
LARGE_TOUCHED = {
    "jspsr_loss_workspace_bytes": touched_loss, "jspsr_loss_valid_workspace_bytes": touched_loss_valid,
    "jspsr_metrics_workspace_bytes": touched_metrics, "jspsr_gate_mlp_backward_workspace_bytes": touched_gate,
    "jspsr_scene_nearest_seed_workspace_bytes": touched_seed,
    # no arguments: the largest launch is the capped one
    "jspsr_optim_workspace_bytes": lambda: touched_optim(1 << 40), "jspsr_tensor_ranges_workspace_bytes": lambda: touched_ranges(8),
}
_BIG = [(8, 512, 512), (64, 1024, 1024), (1, 46340, 46340), (65535, 4096, 4095)]        # the last: the most planes, 2^40 - 2^28 elements
LARGE["jspsr_loss_menu_workspace_bytes"] = [(t,) + s for t in (7, 8, 15) for s in _BIG]
LARGE["jspsr_loss_menu_valid_workspace_bytes"] = [(7,) + s for s in _BIG]
LARGE["jspsr_loss_menu_valid_ssim_workspace_bytes"] = [(t,) + s + (1,) for t in (7, 8, 15) for s in _BIG]
LARGE["jspsr_ssim_workspace_bytes"] = [s + (m,) for m in (0, 1) for s in _BIG]
LARGE["jspsr_ssim_tiles_workspace_bytes"] = [s + (b, m) for m in (0, 1) for b in (0.0, 0.05) for s in _BIG]
LARGE_TOUCHED.update({
    "jspsr_loss_menu_workspace_bytes": touched_menu, "jspsr_loss_menu_valid_workspace_bytes": touched_menu_valid,
    "jspsr_loss_menu_valid_ssim_workspace_bytes": touched_menu_valid_ssim, "jspsr_ssim_workspace_bytes": touched_ssim,
    "jspsr_ssim_tiles_workspace_bytes": touched_ssim_tiles})
_TILES = [(8, 512, 512), (64, 1024, 1024), (1, 32767, 32767), (65535, 143, 142), (3, 1, 1)]
LARGE["jspsr_scores_batch_workspace_bytes"] = LARGE["jspsr_scores_batch_valid_workspace_bytes"] = _TILES[:4]
LARGE_TOUCHED["jspsr_scores_batch_workspace_bytes"] = lambda *a: touched_scores(0, *a)
LARGE_TOUCHED["jspsr_scores_batch_valid_workspace_bytes"] = lambda *a: touched_scores(1, *a)
_POOLS = [(8, 1, 8 * 512 * 512, 256), (8, 64, 64 * 1024 * 1024, 8192 + 64), (1, 1, 16384 * 16384, 32768), (8, 3, 2 ** 32 - 1, 524287 + 3)]
LARGE["jspsr_summary_workspace_bytes"] = LARGE["jspsr_summary_valid_workspace_bytes"] = _POOLS
LARGE_TOUCHED["jspsr_summary_workspace_bytes"] = lambda *a: touched_summary(0, *a)
LARGE_TOUCHED["jspsr_summary_valid_workspace_bytes"] = lambda *a: touched_summary(1, *a)
LARGE["jspsr_strata_workspace_bytes"] = [(8, 32, 8 * 512 * 512), (8, 5, 64 * 1024 * 1024), (1, 1, 16384 * 16384), (8, 32, 2 ** 32 - 1)]
LARGE_TOUCHED["jspsr_strata_workspace_bytes"] = touched_strata
LARGE["jspsr_errdist_workspace_bytes"] = [(8, 65535), (8, 200)]
LARGE_TOUCHED["jspsr_errdist_workspace_bytes"] = touched_errdist
_RASTERS = [(8, 512, 512), (64, 1024, 1024), (1, 16384, 16384), (8, 513, 515), (4097, 1, 3), (1, 8 * 4097, 3)]
LARGE["jspsr_prop_backward_workspace_bytes"] = LARGE["jspsr_prop_head_backward_workspace_bytes"] = _RASTERS
LARGE["jspsr_prop_step_backward_workspace_bytes"] = _RASTERS
LARGE_TOUCHED["jspsr_prop_backward_workspace_bytes"] = lambda *a: max(touched_prop(e, *a, env) for e in ("planar", "logits") for env in [{}] + PROP_FORMS)
LARGE_TOUCHED["jspsr_prop_head_backward_workspace_bytes"] = lambda *a: max(touched_prop(e, *a, env) for e in ("head_f32", "head_bf16") for env in [{}] + PROP_FORMS)
LARGE_TOUCHED["jspsr_prop_step_backward_workspace_bytes"] = touched_step
LARGE["jspsr_conv2d_wgrad_workspace_bytes"] = [(d, 8, 512, 512, c, c, k, k) for d in (F32, BF16) for c, k in ((64, 3), (256, 1), (32, 3))] + \
                                              [(F32, 64, 1024, 1024, 64, 64, 3, 3), (BF16, 1, 16384, 16384, 32, 32, 3, 3)]
LARGE_TOUCHED["jspsr_conv2d_wgrad_workspace_bytes"] = lambda *a: max(touched_wgrad(*a), touched_wgrad(*a, nine_tap=a[6] == 3))
LARGE["jspsr_bn_backward_pair_workspace_bytes"] = [(F32, 64), (BF16, 2048), (F32, 8192)]
LARGE_TOUCHED["jspsr_bn_backward_pair_workspace_bytes"] = lambda dt, C: max(touched_bn_pair(dt, C, n) for n in (8 * 512 * 512, 64 * 1024 * 1024, 1 << 40))
# queries sized as a maximum over entries this table does not drive: their spare bytes are not bounded here
SHARED_MAX = {"jspsr_bn_backward_pair_workspace_bytes": "jspsr_reduce_workspace_bytes' maximum (the BatchNorm forward's 256-row fold) + 2 C"}
LARGE["jspsr_optim_workspace_bytes"] = [()]
LARGE["jspsr_tensor_ranges_workspace_bytes"] = [()]

# per query: arguments the header lists as bad -> 0
ZERO = {
    "jspsr_loss_workspace_bytes": [(0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8)],
    "jspsr_loss_valid_workspace_bytes": [(0, 8, 8), (8, 0, 8), (8, 8, 0), (8, -2, 8)],
    "jspsr_metrics_workspace_bytes": [(0, 8), (8, 0), (-3, 8)],
    "jspsr_gate_mlp_backward_workspace_bytes": [(0, 64, 4), (1, 0, 4), (1, 64, 0), (1, 16129, 128), (1, 16384, 1)],
    "jspsr_scene_nearest_seed_workspace_bytes": [(0,), (-5,)],
    "jspsr_loss_menu_workspace_bytes": [(0, 1, 12, 12), (16, 1, 12, 12), (-1, 1, 12, 12), (7, 0, 12, 12), (7, 65536, 1, 1), (7, 1, 0, 12),
                                        (7, 1, 12, 0), (8, 1, 10, 12), (8, 1, 12, 10)],
    "jspsr_loss_menu_valid_workspace_bytes": [(0, 1, 12, 12), (8, 1, 12, 12), (15, 1, 12, 12), (16, 1, 12, 12), (7, 0, 12, 12), (7, 1, 0, 12)],
    "jspsr_loss_menu_valid_ssim_workspace_bytes": [(15, 1, 12, 12, 0), (15, 1, 12, 12, 2), (8, 1, 10, 12, 1), (8, 1, 12, 10, 1),
                                                   (0, 1, 12, 12, 1), (16, 1, 12, 12, 1), (7, 0, 12, 12, 1)],
    "jspsr_ssim_workspace_bytes": [(0, 12, 12, 0), (1, 10, 12, 0), (1, 12, 10, 0), (65536, 12, 12, 1), (1, 0, 12, 1)],
    "jspsr_ssim_tiles_workspace_bytes": [(0, 12, 12, 0.0, 0), (1, 12, 12, 0.5, 0), (1, 12, 12, -0.1, 0), (1, 12, 12, float("nan"), 1),
                                         (1, 12, 14, 0.1, 0), (1, 10, 12, 0.0, 0)],
}
ZERO["jspsr_scores_batch_workspace_bytes"] = ZERO["jspsr_scores_batch_valid_workspace_bytes"] = [
    (0, 8, 8), (1, 2, 8), (1, 8, 2), (1, 0, 8), (-1, 8, 8), (1, 32768, 32768)]

ZERO["jspsr_summary_workspace_bytes"] = ZERO["jspsr_summary_valid_workspace_bytes"] = [
    (0, 1, 35, 1), (9, 1, 35, 1), (1, 0, 35, 1), (1, 1, 0, 1), (1, 1, 2 ** 32, 524288), (1, 36, 35, 36), (1, 1, 8193, 1), (1, 1, 35, 3)]
ZERO["jspsr_strata_workspace_bytes"] = [(0, 1, 35), (9, 1, 35), (1, 0, 35), (1, 33, 35), (1, 1, 0), (1, 1, 2 ** 32)]
ZERO["jspsr_errdist_workspace_bytes"] = [(0, 200), (9, 200), (1, 1), (1, 0), (1, 65536)]

ZERO["jspsr_prop_backward_workspace_bytes"] = ZERO["jspsr_prop_head_backward_workspace_bytes"] = [(0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)]
ZERO["jspsr_prop_step_backward_workspace_bytes"] = [(0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)]

ZERO["jspsr_conv2d_wgrad_workspace_bytes"] = [(F32, 0, 5, 5, 8, 12, 1, 1), (F32, 1, 0, 5, 8, 12, 1, 1), (F32, 1, 5, 5, 0, 12, 1, 1),
                                              (F32, 1, 5, 5, 8, 0, 1, 1), (F32, 1, 5, 5, 8, 12, 0, 1), (BF16, 1, 5, -1, 8, 16, 1, 1)]
ZERO["jspsr_bn_backward_pair_workspace_bytes"] = [(F32, 0), (BF16, -8)]
