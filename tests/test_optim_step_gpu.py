"""The optimizer kernels on the MI355X, element by element: K11 (`optim_kernel<K, MOM, RANGE>`, csrc/optim.hip: six forms,
with and without the fused gradient range, scalars as arguments and from device memory) and the AdamW kernels
(`jspsr_adamw_step`, `jspsr_adamw_step_dev`, csrc/train_step.hip), called through the raw C entries, against the fp64
restatement of tests/optim_step_ref.py.

Bounds (tests/test_optim_step_cpu.py establishes both on the CPU).  SGD, both forms: the operands make every intermediate an
fp32 dyadic, so the result must equal the fp32 cast of the reference bit for bit.  The other kinds, per case and buffer:
|kernel - step64| <= 4 d + ulp32(max|ref|) at every element, d = max|step32 - step64| of that case and buffer; the factor 4 is
the project's allowance for an equally valid operation order (a fused multiply-add, a reciprocal for a division).  Every
planted mistake stands >= 100 such bounds away.

Run-ahead (the last two tests): steps issued while the stream is still busy with earlier work -- the host several steps
ahead of the GPU, as between the one synchronisation per epoch of `train_one_epoch` -- must leave the bits of steps that
were synchronised one by one.  The stream is kept busy for >= 10 x the measured issue time of the steps, and an event behind
that work must still be pending when the last step call returns: otherwise the test FAILS (it proves nothing then).
With `upload_hyper()` rewriting ONE pinned row per call, as it did before these tests, all seven were red with the stream
proven busy: every queued copy read the row of the last step issued (GraphedStep: the loss of the second replay already
differed, 0.059367 for 0.055527 -- the first replay had stepped with a later row).
"""
import math
import time

import numpy as np
import pytest
import torch

from jspsr_amd import _lib
from jspsr_amd import optim as O
from jspsr_amd.ddp import GradReducer
from tests import optim_step_ref as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORM_IDS = [X.form_name(*f) for f in X.FORMS]
NAN_BITS = 0x7FC0BEEF                      # what the guard floats hold: a NaN pattern no kernel computes
EINVAL, EALIGN = -1, -2
CENSUS = (b"optim_step", b"optim_step (range)", b"adamw_step")


def stream():
    return torch.cuda.current_stream().cuda_stream


def census():
    lib = _lib.load()
    return [lib.jspsr_launch_count(n) for n in CENSUS]


def workspace():
    return torch.empty(_lib.load().jspsr_optim_workspace_bytes() // 4, dtype=torch.float32, device=DEV)


def allocations(case, ops):
    """The four buffers as device tensors of GUARD + mis + n + GUARD floats, NaN-filled outside [GUARD + mis, GUARD + mis + n);
    torch's allocations start 16-byte aligned, so the slice starts `mis` floats off a boundary."""
    total = 2 * X.GUARD + case.mis + case.n
    lo = X.GUARD + case.mis
    out = []
    for a in ops:
        host = np.full(total, NAN_BITS, dtype=np.uint32).view(np.float32)
        host[lo:lo + case.n] = a
        out.append(torch.from_numpy(host).to(DEV))
        assert out[-1].data_ptr() % 16 == 0
    return out, slice(lo, lo + case.n)


def launch(entry, case, bufs, sl, use_hyper, rng, ws, r=None):
    """One raw call; returns the C entry's code.  entry: "optim" | "adamw" | "adamw_dev"."""
    lib = _lib.load()
    r = [X.f32(x) for x in (r if r is not None else X.row(case.kind, case.mom, case.step))]
    u1, u2 = X.owns(case.kind, case.mom)
    p, g, s1, s2 = (b[sl].data_ptr() for b in bufs)
    hyper = torch.tensor(r + [0.0], dtype=torch.float64).float().to(DEV) if use_hyper or entry == "adamw_dev" else None
    if entry == "adamw":
        return lib.jspsr_adamw_step(p, g, s1, s2, case.n, r[0], r[1], r[2], r[3], r[4], case.step, stream())
    if entry == "adamw_dev":
        return lib.jspsr_adamw_step_dev(p, g, s1, s2, case.n, hyper.data_ptr(), stream())
    ptr = lambda t: None if t is None else t.data_ptr()
    if use_hyper:
        return lib.jspsr_optim_step(case.kind, p, g, s1 if u1 else None, s2 if u2 else None, case.n, 0.0, 0.0, 0.0, 0.0, 0.0, 0,
                                    hyper.data_ptr(), ptr(rng), ptr(ws), stream())
    return lib.jspsr_optim_step(case.kind, p, g, s1 if u1 else None, s2 if u2 else None, case.n, r[0], r[1], r[2], r[3], r[4],
                                case.step, None, ptr(rng), ptr(ws), stream())


def run(entry, case, res, use_hyper=False, use_range=False, ws=None):
    """Launch on fresh allocations; returns the four whole allocations afterwards (numpy fp32) and the slice."""
    bufs, sl = allocations(case, res.ops)
    rng = torch.tensor([999.0, -999.0, 0.0, 0.0], device=DEV) if use_range else None
    code = launch(entry, case, bufs, sl, use_hyper, rng, ws if use_range else None)
    assert code == 0, (entry, case, code, _lib.load().jspsr_last_error())
    if use_range:
        g = res.ops[1]
        assert rng.tolist() == [float(g.min()), float(g.max()), 0.0, 0.0], (entry, case)
    return [b.cpu().numpy() for b in bufs], sl


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(what, case, res, after, sl):
    """Every element of P, S1, S2 against the reference; the guards, the gradient and unowned buffers bit-unchanged."""
    total = after[0].shape[0]
    outside = np.ones(total, dtype=bool)
    outside[sl] = False
    for k, name in enumerate(("P", "G", "S1", "S2")):
        assert np.all(bits(after[k])[outside] == NAN_BITS), (what, case, name, "written outside [mis, mis + n)",
                                                             np.flatnonzero(bits(after[k])[outside] != NAN_BITS)[:8])
    assert np.array_equal(bits(after[1][sl]), bits(res.ops[1])), (what, case, "the gradient was written")
    for k, name, idx in ((0, "P", 0), (1, "S1", 2), (2, "S2", 3)):
        got, ref = after[idx][sl], res.ref[k]
        if ref is None:
            assert np.array_equal(bits(got), bits(res.ops[idx])), (what, case, name, "is not this form's, but was written")
            continue
        if res.exact:
            want = ref.astype(np.float32)
            if not torch.equal(torch.from_numpy(got.copy()), torch.from_numpy(want)):
                i = int(np.flatnonzero(got != want)[0])
                raise AssertionError((what, case, name, "first differing element", i, float(got[i]), float(want[i])))
            continue
        err = np.abs(got.astype(np.float64) - ref)
        i = int(np.argmax(err))
        assert err[i] <= res.bound[k], (what, case, name, "worst element", i, float(got[i]), float(ref[i]), float(err[i]),
                                        "bound", res.bound[k], "d", res.d[k])


def variants(kind):
    """(entry, scalars from device memory, fused range) of every kernel that computes this kind."""
    v = [("optim", h, r) for h in (False, True) for r in (False, True)]
    if kind == X.ADAMW:
        v += [("adamw", False, False), ("adamw_dev", True, False)]
    return v


# ---- 1, 2: every element of every instantiation; nothing outside the range is written ---------------------------------------
@pytest.mark.parametrize("kind,mom", X.FORMS, ids=FORM_IDS)
def test_every_element_of_every_kernel_small_sizes(kind, mom):
    ws = workspace()
    worst = [0.0, 0.0, 0.0]                     # largest error / bound per buffer, for the record
    for case in X.small_cases(kind, mom):
        res = X.evaluate_small(case)
        for entry, use_hyper, use_range in variants(kind):
            after, sl = run(entry, case, res, use_hyper, use_range, ws)
            check((entry, use_hyper, use_range), case, res, after, sl)
            if not res.exact:
                for k, idx in ((0, 0), (1, 2), (2, 3)):
                    if res.ref[k] is not None:
                        worst[k] = max(worst[k], float(np.abs(after[idx][sl].astype(np.float64) - res.ref[k]).max()) / res.bound[k])
    print(f"{X.form_name(kind, mom)}: largest |kernel - step64| / bound over the small cases: P {worst[0]:.3f}  S1 {worst[1]:.3f}  S2 {worst[2]:.3f}")


@pytest.mark.parametrize("kind,mom", X.FORMS, ids=FORM_IDS)
def test_every_element_past_one_grid_pass(kind, mom):
    """n = one pass + 5 and two passes + 3 * 1024 + 2: the grid-stride loop's second and third trip.  The first size goes through
    the argument form without the range (and jspsr_adamw_step), the second through the device form with it (and
    jspsr_adamw_step_dev)."""
    ws = workspace()
    first, second = X.wrap_cases(kind, mom)
    plan = [(first, "optim", False, False), (second, "optim", True, True)]
    if kind == X.ADAMW:
        plan += [(first, "adamw", False, False), (second, "adamw_dev", True, False)]
    cache = {}
    for case, entry, use_hyper, use_range in plan:
        res = cache.get(case) or cache.setdefault(case, X.evaluate(case))
        after, sl = run(entry, case, res, use_hyper, use_range, ws)
        check((entry, use_hyper, use_range), case, res, after, sl)


# ---- 3: three spellings of AdamW, one result ------------------------------------------------------------------------------
def test_adamw_spellings_give_the_same_bits():
    """K11 with JSPSR_OPT_ADAMW (arguments, device row, with the range), jspsr_adamw_step and jspsr_adamw_step_dev: the header
    promises the same arithmetic "expression for expression", so the same bits -- on misaligned ranges and past a grid pass."""
    ws = workspace()
    cases = [X.Case(X.ADAMW, True, 1023, 3, 2), X.Case(X.ADAMW, True, 4 * 1024 + 1, 1, 1000), X.Case(X.ADAMW, True, 7, 2, 1),
             X.Case(X.ADAMW, True, X.WRAP_SIZES[0], 3, 2), X.Case(X.ADAMW, True, X.WRAP_SIZES[1], 1, X.ADAM_LATE)]
    for case in cases:
        ops = X.operands(case)
        res = X.Result(ops, None, None, None, None, False)
        first = None
        for entry, use_hyper, use_range in variants(X.ADAMW):
            after, sl = run(entry, case, res, use_hyper, use_range, ws)
            if first is None:
                first = after
                assert not np.array_equal(bits(after[0][sl]), bits(ops[0]))
                continue
            for name, a, b in zip("PGMV", first, after):
                same = bits(a) == bits(b)
                assert same.all(), (case, entry, use_hyper, use_range, name, "first differing element", int(np.flatnonzero(~same)[0]) - sl.start)


# ---- 4: misaligned ranges through the public classes ---------------------------------------------------------------------
class Odd(torch.nn.Module):
    """Four tensors whose flat ranges start off the 16-byte grid.  GradReducer lays the parameters out in REVERSE order, so
    they are declared 6, 1001, 7, 5: the flat buffers hold 5 | 7 | 1001 | 6 elements.  `second` (the 7) is the second lr group:
    its range starts at element 5 (head 3), and the first group's second range at element 12 (head 0)."""

    def __init__(self, seed=0, dtype=torch.float32):
        super().__init__()
        rs = np.random.RandomState(seed)
        mk = lambda *s: torch.nn.Parameter(torch.from_numpy(rs.standard_normal(s)).to(dtype))
        self.last, self.third, self.second, self.first = mk(6), mk(7, 143), mk(7), mk(5)


CLASSES = {"SGD": (O.FlatSGD, torch.optim.SGD, ("momentum_buffer",)), "Adam": (O.FlatAdam, torch.optim.Adam, ("exp_avg", "exp_avg_sq")),
           "AdamW": (O.FlatAdamW, torch.optim.AdamW, ("exp_avg", "exp_avg_sq")),
           "RMSprop": (O.FlatRMSprop, torch.optim.RMSprop, ("square_avg", "momentum_buffer"))}
CONFIGS = [("SGD", 0.0), ("SGD", 0.9), ("Adam", None), ("AdamW", None), ("RMSprop", 0.0), ("RMSprop", 0.9)]
CONFIG_IDS = [n + ("" if m is None else f"-m{m}") for n, m in CONFIGS]


def class_kwargs(name, momentum):
    """The same values for the flat class and for torch.  The decay rates (betas, alpha) are fp32 numbers: the C entries take
    them as floats and form 1 - beta from that float, torch forms it from the double it was given.  For a rate that fp32 does
    not hold the two weights differ -- 1 - float(0.99) is 9.5e-7 below float(0.01), 1 - float(0.999) 1.3e-5 below
    float(0.001) -- which is a difference of hyper-parameters (beta moved by 1e-8), not of the kernel's arithmetic; measured
    here with torch's defaults instead: RMSprop's momentum buffer 1.53e-5 from torch's at |buffer| <= 27 (8 ulp) against a
    bound of 1.27e-5, every other buffer inside its bound."""
    kw = {"lr": 1e-2 if name == "SGD" else 1e-3, "weight_decay": 1e-2}
    if momentum is not None:
        kw["momentum"] = momentum
    if name in ("Adam", "AdamW"):
        kw["betas"] = (X.f32(0.9), X.f32(0.999))
    if name == "RMSprop":
        kw["alpha"] = X.f32(0.99)
    return kw


def odd_grads(step, seed=41):
    rs = np.random.RandomState(seed + step)
    return [torch.from_numpy(rs.standard_normal(s) * 0.1).float() for s in ((6,), (7, 143), (7,), (5,))]


def torch_odd(name, momentum, steps, dtype):
    net = Odd(dtype=dtype)
    opt = CLASSES[name][1]([{"params": [net.last, net.third, net.first]}, {"params": [net.second], "lr": 3e-4}],
                           **class_kwargs(name, momentum))
    for i in range(steps):
        for p, g in zip(net.parameters(), odd_grads(i)):
            p.grad = g.to(dtype)
        opt.step()
    state = [{k: opt.state[p][k].detach().clone() for k in CLASSES[name][2] if opt.state[p].get(k) is not None} for p in net.parameters()]
    return [p.detach().clone() for p in net.parameters()], state


def flat_odd(name, momentum, device_hyper=False):
    net = Odd().to(DEV)
    red = GradReducer(net.parameters())
    opt = CLASSES[name][0](red, lr_overrides={net.second: 3e-4}, **class_kwargs(name, momentum))
    assert opt.flat_p.data_ptr() % 16 == 0 and red.flat.data_ptr() % 16 == 0
    assert [g["ranges"] for g in opt.param_groups] == [[[0, 5], [12, 1019]], [[5, 12]]]
    if device_hyper:
        opt.enable_device_hyper()
    return net, red, opt


@pytest.mark.parametrize("name,momentum", CONFIGS, ids=CONFIG_IDS)
def test_flat_classes_on_misaligned_ranges_match_torch(name, momentum):
    """Ranges starting at elements 5 (head 3) and 12: parameters AND every state buffer after 3 steps against torch.optim,
    under test_flat_optimizer_matches_torch's bound: max|flat - torch32| <= 4 max|torch32 - torch64| + 1e-7 per tensor, and
    rtol 1e-5 / atol 1e-7."""
    t32, s32 = torch_odd(name, momentum, 3, torch.float32)
    t64, s64 = torch_odd(name, momentum, 3, torch.float64)
    for device_hyper in (False, True):
        net, red, opt = flat_odd(name, momentum, device_hyper)
        for i in range(3):
            opt.zero_grad()
            for p, g in zip(net.parameters(), odd_grads(i)):
                p.grad.copy_(g)
            red.finish()
            opt.step()
        for k, p in enumerate(net.parameters()):
            off, n = opt._slices[id(p)]
            pairs = [("param", p.detach().cpu(), t32[k], t64[k])]
            for key in CLASSES[name][2]:
                buf = getattr(opt, key, None)
                assert (buf is not None) == (key in s32[k]), (name, key)
                if buf is not None:
                    pairs.append((key, buf[off:off + n].cpu().view_as(p), s32[k][key], s64[k][key]))
            for key, got, a, b in pairs:
                ref_err = (a.double() - b).abs().max().item()
                err = (got - a).abs().max().item()
                print(f"{name} m={momentum} dev={device_hyper} tensor {k} {key}: |flat-torch32| {err:.3e}  |torch32-torch64| {ref_err:.3e}")
                assert err <= 4 * ref_err + 1e-7, (name, k, key, err, ref_err)
                assert torch.allclose(got, a, rtol=1e-5, atol=1e-7), (name, k, key)


# ---- 5: refusals launch nothing ------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_launch_nothing():
    lib = _lib.load()
    n = 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    base = [torch.randn(n + 8, device=DEV, generator=gen) for _ in range(4)]
    base[3].abs_()
    rng, ws = torch.tensor([999.0, -999.0, 0.0, 0.0], device=DEV), workspace()
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 0.0316, 0.0], device=DEV)
    keep = [t.clone() for t in base + [rng, hyper]]
    p, g, s1, s2 = (t.data_ptr() for t in base)
    s = stream()
    adam = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
    optim = lambda kind, p_, g_, a_, b_, n_, step, hy, r_, w_: lib.jspsr_optim_step(kind, p_, g_, a_, b_, n_, *adam, step, hy, r_, w_, s)
    refusals = [
        ("unknown kind 4", EINVAL, lambda: optim(4, p, g, s1, s2, n, 1, None, None, None)),
        ("unknown kind -1", EINVAL, lambda: optim(-1, p, g, s1, s2, n, 1, None, None, None)),
        ("n = 0", EINVAL, lambda: optim(2, p, g, s1, s2, 0, 1, None, None, None)),
        ("n < 0", EINVAL, lambda: optim(2, p, g, s1, s2, -4, 1, None, None, None)),
        ("n = 0, adamw_step", EINVAL, lambda: lib.jspsr_adamw_step(p, g, s1, s2, 0, *adam, 1, s)),
        ("n = 0, adamw_step_dev", EINVAL, lambda: lib.jspsr_adamw_step_dev(p, g, s1, s2, 0, hyper.data_ptr(), s)),
        ("step = 0 without hyper", EINVAL, lambda: optim(1, p, g, s1, s2, n, 0, None, None, None)),
        ("step < 0 without hyper", EINVAL, lambda: optim(0, p, g, s1, None, n, -1, None, None, None)),
        ("step = 0, adamw_step", EINVAL, lambda: lib.jspsr_adamw_step(p, g, s1, s2, n, *adam, 0, s)),
        ("SGD with state2", EINVAL, lambda: optim(0, p, g, s1, s2, n, 1, None, None, None)),
        ("SGD with state2 alone", EINVAL, lambda: optim(0, p, g, None, s2, n, 1, None, None, None)),
        ("Adam without state2", EINVAL, lambda: optim(1, p, g, s1, None, n, 1, None, None, None)),
        ("AdamW without state2, device row", EINVAL, lambda: optim(2, p, g, s1, None, n, 0, hyper.data_ptr(), None, None)),
        ("RMSprop without state1", EINVAL, lambda: optim(3, p, g, None, s2, n, 1, None, None, None)),
        ("grad_range without a workspace", EINVAL, lambda: optim(2, p, g, s1, s2, n, 1, None, rng.data_ptr(), None)),
        ("gradient at another offset", EALIGN, lambda: optim(2, p, g + 4, s1, s2, n, 1, None, None, None)),
        ("state1 at another offset", EALIGN, lambda: optim(2, p + 8, g + 8, s1 + 12, s2 + 8, n, 1, None, None, None)),
        ("state2 at another offset, adamw_step", EALIGN, lambda: lib.jspsr_adamw_step(p + 4, g + 4, s1 + 4, s2, n, *adam, 1, s)),
        ("parameters at another offset, adamw_step_dev", EALIGN, lambda: lib.jspsr_adamw_step_dev(p + 4, g, s1, s2, n, hyper.data_ptr(), s)),
        ("2-byte misaligned buffers", EALIGN, lambda: optim(2, p + 2, g + 2, s1 + 2, s2 + 2, n, 1, None, None, None)),
        ("2-byte misaligned buffers, adamw_step", EALIGN, lambda: lib.jspsr_adamw_step(p + 2, g + 2, s1 + 2, s2 + 2, n, *adam, 1, s)),
        ("2-byte misaligned device row", EALIGN, lambda: lib.jspsr_adamw_step_dev(p, g, s1, s2, n, hyper.data_ptr() + 2, s)),
    ]
    for what, want, call in refusals:
        before = census()
        code = call()
        assert code == want, (what, code, lib.jspsr_last_error())
        assert census() == before, (what, "a kernel was launched")
        torch.cuda.synchronize()
        for t, k in zip(base + [rng, hyper], keep):
            assert torch.equal(t, k), (what, "a buffer was written")
    before = census()                          # and the census does count what IS launched
    assert optim(2, p + 4, g + 4, s1 + 4, s2 + 4, n, 1, None, rng.data_ptr(), ws.data_ptr()) == 0
    assert lib.jspsr_adamw_step(p, g, s1, s2, n, *adam, 1, s) == 0
    assert [a - b for a, b in zip(census(), before)] == [1, 1, 1]


# ---- 6: steps issued without synchronisation equal synchronised steps ----------------------------------------------------
BUSY_CAP_MS = 2000.0


class Busy:
    """Plain torch work that keeps the current stream occupied: passes of an element-wise update over 512 MB."""

    def __init__(self):
        self.x = torch.ones(128 << 20, dtype=torch.float32, device=DEV)
        self.pass_ms = None

    def one(self):
        self.x.mul_(1.0000001).add_(1e-9)

    def measure(self):
        for _ in range(3):
            self.one()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            self.one()
        b.record()
        torch.cuda.synchronize()
        self.pass_ms = a.elapsed_time(b) / 10
        return self.pass_ms

    def enqueue(self, issue_ms):
        """>= 10 x the issue time (and >= 50 ms), at most BUSY_CAP_MS; returns (an event recorded behind it, its length in ms)."""
        want_ms = min(BUSY_CAP_MS, max(10.0 * issue_ms, 50.0))
        passes = max(1, math.ceil(want_ms / self.pass_ms))
        for _ in range(passes):
            self.one()
        ev = torch.cuda.Event()
        ev.record()
        return ev, passes * self.pass_ms


@pytest.fixture(scope="module")
def busy():
    b = Busy()
    b.measure()
    return b


K_EAGER = 6
LRS = [1e-2, 2.5e-3, 7e-3, 1e-3, 4e-3, 5e-4]               # opt.lr before each step: every row differs from the one before


def eager_steps(name, momentum, staged, busy, issue_ms=None):
    """K_EAGER steps with the scalars in device memory.  issue_ms None: synchronise after every step (the reference run),
    return the host's issue time.  Otherwise: keep the stream busy first and never synchronise until the end."""
    net, red, opt = flat_odd(name, momentum, device_hyper=True)
    torch.cuda.synchronize()
    ev = busy_ms = None
    if issue_ms is not None:
        ev, busy_ms = busy.enqueue(issue_ms)
    spent = 0.0
    for k in range(K_EAGER):
        t0 = time.perf_counter()
        opt.lr = LRS[k]
        red.flat.copy_(staged[k])                  # device to device: nothing here waits for the GPU
        opt.step()
        spent += time.perf_counter() - t0
        if issue_ms is None:
            torch.cuda.synchronize()
    still_busy = None if ev is None else not ev.query()
    torch.cuda.synchronize()
    state = {key: getattr(opt, key).clone() for key in CLASSES[name][2] if getattr(opt, key, None) is not None}
    return opt.flat_p.clone(), state, spent * 1e3, busy_ms, still_busy


@pytest.mark.parametrize("name,momentum", CONFIGS, ids=CONFIG_IDS)
def test_eager_device_hyper_steps_survive_run_ahead(name, momentum, busy):
    gen = torch.Generator(device=DEV).manual_seed(77)
    staged = [torch.randn(1019, device=DEV, generator=gen) * 0.1 for _ in range(K_EAGER)]
    ref_p, ref_s, issue_ms, _, _ = eager_steps(name, momentum, staged, busy)
    got_p, got_s, ahead_ms, busy_ms, still_busy = eager_steps(name, momentum, staged, busy, issue_ms)
    print(f"{name} m={momentum}: issue of {K_EAGER} steps {issue_ms:.3f} ms synchronised, {ahead_ms:.3f} ms running ahead; "
          f"busy work {busy_ms:.1f} ms ({busy.pass_ms:.3f} ms per pass)")
    assert still_busy, (f"the stream had drained before the last step was issued (busy work {busy_ms:.1f} ms, issue {ahead_ms:.3f} ms): "
                        "the run-ahead was not exercised")
    same = got_p == ref_p
    assert same.all(), (name, "parameters differ from the synchronised run; first element", int((~same).nonzero()[0]))
    assert set(got_s) == set(ref_s)
    for key in ref_s:
        assert torch.equal(got_s[key], ref_s[key]), (name, key)


def test_graphed_step_replays_survive_run_ahead(busy):
    """GraphedStep over JSPSR nf 8 at 2 x 64 x 64 in fp32 with FlatAdamW: 3 warm-up steps, then 5 replays with the learning rate
    changed before every one.  Replays issued back to back behind busy work must give the losses, parameters, buffers and
    moments of replays synchronised one by one."""
    from jspsr_amd.JSPSR import Model
    from jspsr_amd.graph import GraphedStep
    from jspsr_amd.losses import MultiLoss
    from oracle import jspsr_ref as R
    ic = {"lr_dem": 1, "image": 3, "mask": 15}
    sd = R.make_state_dict(R.jspsr_param_shapes(ic, 8), seed=21)
    inp, gt = R.synthetic_batch(2, 64, 64, True, seed=22)
    inp, gt = [t.to(DEV) for t in inp], gt.to(DEV)
    lrs = [1e-3, 2.5e-4, 7e-4, 1e-4, 4e-4]

    def replays(issue_ms=None):
        m = Model(dict(ic, COP30=1), num_feature=8)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        m.compute_dtype = torch.float32
        red = GradReducer(m.parameters())
        red.watch_streams(m.side_streams("cuda"))
        opt = O.FlatAdamW(red, lr=1e-3, weight_decay=1e-6)
        step = GraphedStep(m, red, opt, MultiLoss(1.0, 1.0, 0.1), inp, gt, warmup=3)
        torch.cuda.synchronize()
        ev = busy_ms = None
        if issue_ms is not None:
            ev, busy_ms = busy.enqueue(issue_ms)
        spent, losses = 0.0, []
        for lr in lrs:
            t0 = time.perf_counter()
            opt.lr = lr
            losses.append(step().clone())          # on the stream, behind the replay
            spent += time.perf_counter() - t0
            if issue_ms is None:
                torch.cuda.synchronize()
        still_busy = None if ev is None else not ev.query()
        torch.cuda.synchronize()
        assert opt.steps == 3 + len(lrs) and step.replays == len(lrs)
        state = {k: v.clone() for k, v in m.state_dict().items()}
        state["exp_avg"], state["exp_avg_sq"] = opt.exp_avg.clone(), opt.exp_avg_sq.clone()
        return [v.item() for v in losses], state, spent * 1e3, busy_ms, still_busy

    ref_losses, ref_state, issue_ms, _, _ = replays()
    losses, state, ahead_ms, busy_ms, still_busy = replays(issue_ms)
    print(f"GraphedStep: issue of {len(lrs)} replays {issue_ms:.3f} ms synchronised, {ahead_ms:.3f} ms running ahead; "
          f"busy work {busy_ms:.1f} ms ({busy.pass_ms:.3f} ms per pass)")
    print(f"GraphedStep: losses synchronised {ref_losses}, running ahead {losses}")
    assert still_busy, (f"the stream had drained before the last replay was issued (busy work {busy_ms:.1f} ms, issue {ahead_ms:.3f} ms): "
                        "the run-ahead was not exercised")
    assert losses == ref_losses, ("first differing replay", [a == b for a, b in zip(losses, ref_losses)].index(False) + 1)
    assert set(state) == set(ref_state)
    for k, v in ref_state.items():
        assert torch.equal(state[k], v), k
