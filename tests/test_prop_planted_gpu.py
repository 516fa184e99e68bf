"""GPU parity of K1 (jspsr_prop_forward/backward_f32), its logits entry (jspsr_prop_logits_*) and K1h
(jspsr_prop_head_*) on the planted cases of tests/prop_planted_ref.py: every gradient element by element against the
fp64 closed form ON the kinks, the raster border and the far taps -- no kink mask anywhere, the coordinates are exact in
fp32 -- with the tolerance taken from the fp32 evaluation of the same reference (`P.atol`, the rule of
tests/test_prop_steps_gpu.py), never from the kernel.

Each case also asserts: grad_offset of a tap without a corner inside the raster is exactly 0 and such a tap contributes
exactly nothing (same bits with the tap moved elsewhere outside); everything is finite; every output is written (NaN
prefill), nothing in the 256 bytes before and behind it is (canaries); K1h's seven padding channels and oc = 18's
centre-tap offset gradient hold the reference's value; the operands keep their bits; two calls give the same bits.

Entries are called through the raw wrappers / the C ABI, so the test owns every output buffer; the path taken (LDS-DMA or
general kernel) is asserted from the launch census.  The sigmoid entries (logits, K1h) get the allowance of
P.logits_refs on top: a relative 2^-21 = 8 ulp on the affinity (one rounding of l * log2 e amplified by |l| ln 2 <= 4.2,
plus one ulp each for v_exp_f32, the add and v_rcp_f32 -- prop_dma.hip, prop.hip and prop_head.hip share that sequence).
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import prop_planted_ref as P

pytestmark = pytest.mark.gpu

CANARY = -17.25                   # exact in bf16 too
GUARD_BYTES = 256
ID = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)

#            name                  kind      oc  dtype            unaligned
ENTRIES = {
    "planar18":            ("planar", 18, torch.float32, False),
    "planar16":            ("planar", 16, torch.float32, False),
    "planar16-unaligned":  ("planar", 16, torch.float32, True),     # pointers aligned to 4 bytes only: general kernel
    "logits":              ("logits", 16, torch.float32, False),
    "logits-unaligned":    ("logits", 16, torch.float32, True),
    "head-f32":            ("head", 16, torch.float32, False),      # always the general kernel
    "head-bf16":           ("head", 16, torch.bfloat16, False),
    "head-bf16-unaligned": ("head", 16, torch.bfloat16, True),      # dem / out / grad_out off by 4 bytes: general kernel
}
CENSUS = {
    "planar": ("prop_forward (dma)", "prop_backward (dma)", "prop_forward", "prop_backward"),
    "logits": ("prop_logits_forward (dma)", "prop_logits_backward (dma)", "prop_logits_forward", "prop_logits_backward"),
    "head": ("prop_head_forward (dma)", "prop_head_backward (dma)", "prop_head_forward", "prop_head_backward"),
}


def _lib():
    from jspsr_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Guarded:
    """An output the test owns: a view into a larger buffer, NaN inside, 256 bytes of canary in front and behind."""

    def __init__(self, shape, dtype=torch.float32, unaligned=False):
        n = 1
        for s in shape:
            n *= s
        self.n, self.front = n, GUARD_BYTES // torch.empty((), dtype=dtype).element_size() + (1 if unaligned else 0)
        self.buf = torch.full((n + 2 * self.front,), CANARY, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.v = self.buf[self.front:self.front + n].view(shape)
        self.v.fill_(float("nan"))
        assert self.v.data_ptr() % 16 == (4 if unaligned else 0) and self.v.is_contiguous()

    def take(self, what):
        """-> CPU copy, after the checks: every element written, nothing written around it."""
        assert bool((self.buf[:self.front] == CANARY).all()), f"{what}: written in front of the output"
        assert bool((self.buf[self.front + self.n:] == CANARY).all()), f"{what}: written behind the output"
        got = self.v.cpu().clone()
        assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} elements NaN (unwritten or computed so)"
        return got


def _operand(t, unaligned=False):
    """A device copy of `t`; unaligned: one float into a larger buffer (4-byte aligned, not 16)."""
    if not unaligned:
        return t.contiguous().cuda()
    buf = torch.empty(t.numel() + 8, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _dma_expected(kind, dtype, W, unaligned):
    if W % 4 or unaligned:
        return False
    if kind == "head":
        return dtype == torch.bfloat16 and os.environ.get("JSPSR_PROP_HEAD_DMA", "1") != "0"
    return os.environ.get("JSPSR_PROP_DMA", "1") != "0"


def _run(c, entry, scale):
    """One forward and one backward of the entry on the case -> dict of CPU tensors (QUANT; K1h also `pad`, the seven unused
    channels of its head gradient), after the checks a single call can make: canaries, NaN prefill, operands untouched,
    path taken."""
    from jspsr_amd import kernels as K
    from jspsr_amd import ops
    kind, oc, dtype, un = ENTRIES[entry]
    assert oc == c["oc"]
    lib = _lib().load()
    B, H, W = c["shape"]
    off = c["offset"] if oc == 18 else P.to16(c["offset"])
    dem, gout = _operand(c["dem"], un), _operand(c["gout"], un)
    wk, b0 = c["wk"].cuda(), c["b0"].cuda()
    if kind == "planar":
        ins = dict(dem=dem, gout=gout, weight=_operand(c["weight"], un), offset=_operand(off, un))
        outs = dict(grad_weight=_Guarded((B, 9, H, W), unaligned=un), grad_offset=_Guarded((B, oc, H, W), unaligned=un))
    elif kind == "logits":
        ins = dict(dem=dem, gout=gout, head=_operand(torch.cat((c["logits"], off), 1), un))
        outs = dict(grad_head=_Guarded((B, 25, H, W), unaligned=un))
    else:
        ins = dict(dem=dem, gout=gout, head=P.pack_head(c["logits"], c["offset"], c["pad"]).to(dtype).cuda())
        outs = dict(grad_head=_Guarded((B, H, W, 32), dtype))
    outs.update(out=_Guarded((B, 1, H, W), unaligned=un), grad_wk=_Guarded((9,)), grad_b0=_Guarded((1,)))
    keep = {k: _bits(v).clone() for k, v in ins.items()}
    names = CENSUS[kind]
    before = [lib.jspsr_launch_count(n.encode()) for n in names]
    if kind == "planar":
        ws = ops.prop_backward_workspace(B, H, W, "cuda")
        ops.prop_forward_raw(dem, ins["weight"], ins["offset"], wk, b0, scale, outs["out"].v)
        ops.prop_backward_raw(gout, dem, ins["weight"], ins["offset"], wk, outs["grad_weight"].v, outs["grad_offset"].v,
                              outs["grad_wk"].v, outs["grad_b0"].v, ws)
    elif kind == "logits":
        ws = ops.prop_backward_workspace(B, H, W, "cuda")
        _lib().check(lib.jspsr_prop_logits_forward_f32(dem.data_ptr(), ins["head"].data_ptr(), wk.data_ptr(), b0.data_ptr(), float(scale),
                                                       outs["out"].v.data_ptr(), B, H, W, _stream()), "jspsr_prop_logits_forward_f32")
        _lib().check(lib.jspsr_prop_logits_backward_f32(gout.data_ptr(), dem.data_ptr(), ins["head"].data_ptr(), wk.data_ptr(),
                                                        outs["grad_head"].v.data_ptr(), outs["grad_wk"].v.data_ptr(),
                                                        outs["grad_b0"].v.data_ptr(), ws.data_ptr(), B, H, W, _stream()),
                     "jspsr_prop_logits_backward_f32")
    else:
        ws = torch.empty(max(lib.jspsr_prop_head_backward_workspace_bytes(B, H, W), 16), dtype=torch.uint8, device="cuda")
        dt = K._dt(ins["head"])
        _lib().check(lib.jspsr_prop_head_forward(dt, dem.data_ptr(), ins["head"].data_ptr(), wk.data_ptr(), b0.data_ptr(), float(scale),
                                                 outs["out"].v.data_ptr(), B, H, W, _stream()), "jspsr_prop_head_forward")
        _lib().check(lib.jspsr_prop_head_backward(dt, gout.data_ptr(), dem.data_ptr(), ins["head"].data_ptr(), wk.data_ptr(),
                                                  outs["grad_head"].v.data_ptr(), outs["grad_wk"].v.data_ptr(),
                                                  outs["grad_b0"].v.data_ptr(), ws.data_ptr(), B, H, W, _stream()),
                     "jspsr_prop_head_backward")
    torch.cuda.synchronize()
    delta = tuple(lib.jspsr_launch_count(n.encode()) - b for n, b in zip(names, before))
    assert delta == ((1, 1, 0, 0) if _dma_expected(kind, dtype, W, un) else (0, 0, 1, 1)), (entry, c["shape"], dict(zip(names, delta)))
    for k, v in ins.items():
        assert torch.equal(_bits(v), keep[k]), f"{entry}: operand {k} was modified"
    res = {k: g.take(f"{entry} {c['shape']} {k}") for k, g in outs.items()}
    if kind == "logits":
        gh = res.pop("grad_head")
        res.update(grad_weight=gh[:, :9], grad_offset=gh[:, 9:])
    elif kind == "head":
        res["grad_head_bits"] = _bits(res["grad_head"])
        res["grad_weight"], res["grad_offset"], res["pad"] = P.unpack_head(res.pop("grad_head").float())
    return res


@functools.lru_cache(maxsize=None)
def _case(shape, oc, bf16, zero=False):
    c = P.case(*shape, oc, P.seed_of(shape, oc, bf16), bf16=bf16)
    if zero:                                                   # what a freshly initialised or collapsed offset head emits
        c = dict(c, offset=torch.zeros_like(c["offset"]))
    return c


@functools.lru_cache(maxsize=None)
def _refs(shape, oc, bf16, sig, scale, zero=False):
    """(fp64, fp32, sigmoid allowance) of one case, computed once and shared by the entries that use it."""
    c = _case(shape, oc, bf16, zero)
    if sig:
        return P.logits_refs(c, scale)
    return P.planar_refs(c, scale) + (dict.fromkeys(P.QUANT, 0.0),)


def _close(got, ref, atol, rtol, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())                     # NaN in `got` is bad
    worst = err.nan_to_num(float("inf")).max().item() if err.numel() else 0.0
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, max err {worst:.3e}, atol {atol:.3e}"
    return worst


def check(entry, shape, zero=False):
    """Everything this file asserts, for one entry on one shape (zero: all offsets exactly 0)."""
    kind, oc, dtype, un = ENTRIES[entry]
    bf16 = dtype == torch.bfloat16
    scale = P.scale_of(shape)
    c = _case(shape, oc, bf16, zero)
    r64, r32, allow = _refs(shape, oc, bf16, kind != "planar", scale, zero)
    got = _run(c, entry, scale)
    # 1. parity, element by element, no mask
    for k in P.QUANT:
        atol, floor = P.atol(r64[k], r32[k], allow[k])
        assert atol <= P.CAPS[k], f"{entry} {shape} {k}: derived atol {atol:.3e} (fp32 floor {floor:.3e}) exceeds {P.CAPS[k]:.1e}"
        rtol = P.RTOL_BF16 if bf16 and k in ("grad_weight", "grad_offset") else P.RTOL      # the head gradient is stored in bf16
        assert bool(torch.isfinite(got[k]).all()), (entry, shape, k)
        err = _close(got[k].reshape(r64[k].shape), r64[k], atol, rtol, f"{entry} {shape} {k}")
        print(f"PLANTED {entry}{'-zero' if zero else ''} {ID(shape)} {k}: fp32 floor {floor:.2e}  sigmoid allowance {allow[k]:.2e}  atol {atol:.2e}  max err {err:.2e}")
    if kind == "head":
        assert bool((got["pad"] == 0).all()), f"{entry} {shape}: padding channels of the head gradient are not 0"
    # 2. taps without a corner inside the raster: grad_offset exactly 0, and exactly no contribution wherever they are
    dead = P.all_corners_outside(c["offset"]).repeat_interleave(2, 1)
    if oc == 16:
        dead = P.to16(dead)
    assert bool((got["grad_offset"][dead] == 0).all()), f"{entry} {shape}: grad_offset of {int((got['grad_offset'][dead] != 0).sum())} outside taps is not 0"
    moved = _run(P.moved_outside(c), entry, scale)
    # 3. the same call again: the same bits
    again = _run(c, entry, scale)
    for k in got:
        assert torch.equal(got[k], moved[k]), f"{entry} {shape} {k}: taps outside the raster contribute something"
        assert torch.equal(_bits(got[k]), _bits(again[k])), f"{entry} {shape} {k}: not reproducible"


def _applies(entry, shape):
    """Unaligned operands make a difference only where the aligned ones take the DMA kernels."""
    return not ENTRIES[entry][3] or (shape[2] % 4 == 0 and shape in ((2, 6, 132), (1, 28, 196)))


@pytest.mark.parametrize("entry,shape", [(e, s) for e in ENTRIES for s in P.SHAPES if _applies(e, s)], ids=ID)
def test_planted_table(entry, shape):
    check(entry, shape)


@pytest.mark.parametrize("shape", [(2, 6, 132), (2, 13, 70)], ids=ID)
@pytest.mark.parametrize("entry", ["planar18", "planar16", "logits", "head-bf16", "head-f32"])
def test_all_offsets_zero(entry, shape):
    """Every tap on a kink in both components: the whole offset gradient is the floor-side convention."""
    check(entry, shape, zero=True)


@pytest.mark.parametrize("entry", ["planar16", "logits", "head-bf16", "head-f32"])
def test_more_tiles_than_workgroups(entry):
    """1 x 260 x 1028: 1105 DMA tiles, persistent runs of several tiles per workgroup, ragged both ways."""
    check(entry, P.BIG)


# ---- the other instantiations: the library reads its switches once, so one child process per setting -------------------
CHILD_SHAPES = [(2, 6, 132), (1, 28, 196), (2, 13, 70)]
GENERAL = {"JSPSR_PROP_DMA": "0", "JSPSR_PROP_HEAD_DMA": "0"}
FORMS = [
    # the forms of the DMA kernels (tests/test_prop_gpu.py lists the same six)
    ({"JSPSR_PROP_SPLIT": "0", "JSPSR_PROP_HEAD_SPLIT": "0"}, True),
    ({"JSPSR_PROP_SPLIT": "1", "JSPSR_PROP_NW": "8"}, False),
    ({"JSPSR_PROP_NTL": "0", "JSPSR_PROP_WGS": "1", "JSPSR_PROP_HEAD_WGS": "1"}, True),
    (GENERAL, True),
    ({"JSPSR_PROP_SPLIT": "0", "JSPSR_PROP_RP": "2"}, False),
    ({"JSPSR_PROP_SPLIT": "0", "JSPSR_PROP_RP": "4"}, False),
    # a covering set of the general kernel's other instantiations (prop.hip by_shape); K1h's general kernel has one form
    (dict(GENERAL, JSPSR_PROP_TH="4"), False),
    (dict(GENERAL, JSPSR_PROP_TH="16"), False),
    (dict(GENERAL, JSPSR_PROP_PX="2"), False),
    (dict(GENERAL, JSPSR_PROP_PX="4"), False),          # VEC = 1 on aligned W % 4 == 0 operands; VEC = 0 on the 4-byte-aligned ones and at W = 70
    (dict(GENERAL, JSPSR_PROP_TW="128", JSPSR_PROP_TH="4"), False),
    (dict(GENERAL, JSPSR_PROP_TW="128", JSPSR_PROP_TH="8"), False),
    (dict(GENERAL, JSPSR_PROP_TW="256", JSPSR_PROP_TH="2"), False),
    (dict(GENERAL, JSPSR_PROP_TW="256", JSPSR_PROP_TH="8"), False),
]


def child_table(heads):
    """What a child process runs: the planted table of the planar 18 / 16 and the logits entry, the 4-byte-aligned
    operands, and K1h where the setting concerns it."""
    for shape in CHILD_SHAPES:
        for entry in ("planar18", "planar16", "logits") + (("head-bf16", "head-f32") if heads else ()):
            check(entry, shape)
    for shape in ((2, 6, 132), (1, 28, 196)):
        check("planar16-unaligned", shape)
    check("logits-unaligned", (2, 6, 132))
    print("planted ok")


@pytest.mark.parametrize("env,heads", FORMS, ids=lambda v: "_".join(f"{k[6:]}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_planted_table_in_other_forms(env, heads):
    code = f"from tests import test_prop_planted_gpu as T; T.child_table({heads})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.stdout.write("".join(f"{env} {line}\n" for line in r.stdout.splitlines() if line.startswith("PLANTED")))
    assert r.returncode == 0 and "planted ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
