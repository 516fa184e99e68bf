"""TEST INFRASTRUCTURE ONLY -- the optimizer kernels' yardstick: K11 (`optim_kernel<K, MOM, RANGE>`, csrc/optim.hip) and the
AdamW kernels (`adamw_kernel`, `adamw_dev_kernel`, csrc/train_step.hip).

* `step64`: ONE update of each of the six (kind, momentum) forms in numpy float64, written from torch.optim's documented
  algorithms (SGD, Adam, AdamW, RMSprop at their defaults: dampening 0, no Nesterov, not centered, no amsgrad), from the
  seven scalars of jspsr_optim_step's documented row { lr, a, b, eps, weight decay, c1, c2 } (include/jspsr_hip.h), rounded
  to fp32 first, as the kernel receives them.  `step32`: the same in numpy float32, one rounding per operation, in the
  expression order the kernel's comment states (no fused multiply-add).
* the cases: every small size x every misalignment x the step counts, the two sizes past one grid pass, and the operands.
* the planted MISTAKES, applied to the reference's output: what an indexing bug or a stale scalar row would leave behind.

Operands.  SGD (both forms): P and S1 odd integers in [-63, 63], G an integer in [-16, 16], lr = 2^-3, weight decay = 2^-4,
momentum = 0.5.  G + P / 16 is a multiple of 1/16 below 20, S1 / 2 + that a multiple of 1/16 below 52, P - that / 8 a
multiple of 2^-7 below 71: every intermediate is a dyadic of at most 14 bits, fp32 holds it, and neither the order nor a
contraction can change the result -- the GPU test demands bit equality.  P and S1 are ODD so that no update is zero (P / 16
keeps an odd numerator over 16 through every sum above): a skipped or a repeated element always shows.
The other kinds: seeded normals folded away from zero and clipped (|P| in [1/4, 4], |G| in [1/4, 2], first moments in
[1/2, 4], second moments in [1/16, 1]) with lr = 2^-3, so that one update (>= 2e-3) stands far above the rounding (~1e-6):
0.9 |exp_avg| >= 0.45 > 0.1 |G|, and 0.81 |exp_avg| >= 0.405 > 0.19 |G| for an element updated twice.

No GPU import here: tests/test_optim_step_cpu.py runs all of it on a machine without one.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

SGD, ADAM, ADAMW, RMSPROP = 0, 1, 2, 3                   # JSPSR_OPT_* of include/jspsr_hip.h
NAMES = {SGD: "SGD", ADAM: "Adam", ADAMW: "AdamW", RMSPROP: "RMSprop"}
FORMS = ((SGD, False), (SGD, True), (ADAM, True), (ADAMW, True), (RMSPROP, False), (RMSPROP, True))

GRID = 4096 * 256 * 4                                    # elements of one grid pass: workgroups x threads x floats
SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 4 * 1024 + 1)
MIS = (0, 1, 2, 3)                                       # floats off a 16-byte boundary
WRAP_SIZES = (GRID + 5, 2 * GRID + 3 * 1024 + 2)
GUARD = 8                                                # floats on each side of [GUARD + mis, GUARD + mis + n)
STEPS = (1, 2, 1000)                                     # SGD's first-step flag and Adam's corrections: 0.1, 0.19, 1 - 2e-46
ADAM_LATE = 10000                                        # 0.9^10000 underflows (also in double): c1 is exactly 1

LR, SGD_WD, SGD_MOMENTUM = 2.0 ** -3, 2.0 ** -4, 0.5
BETAS, ADAM_EPS, WD = (0.9, 0.999), 1e-8, 1e-2
ALPHA, RMS_MOMENTUM, RMS_EPS = 0.99, 0.9, 1e-8

Case = namedtuple("Case", "kind mom n mis step")


def form_name(kind, mom):
    return NAMES[kind] + ("+momentum" if mom and kind in (SGD, RMSPROP) else "")


def owns(kind, mom):
    """(does the form own state1, does it own state2)"""
    return (kind != SGD or mom, kind in (ADAM, ADAMW) or (kind == RMSPROP and mom))


def steps_of(kind):
    return STEPS + ((ADAM_LATE,) if kind in (ADAM, ADAMW) else ())


def small_cases(kind, mom):
    return [Case(kind, mom, n, mis, step) for n in SIZES for mis in MIS for step in steps_of(kind)]


def wrap_cases(kind, mom):
    """Both sizes once per form; mis alternates between 1 and 3 across the forms, the step counts differ.  GRID + 5 at mis 1
    (head 3) fills ONE pass to its last float4 and leaves a tail of 2 -- the loop's bound itself --, at mis 3 (head 1) a single
    float4 starts the second pass; the second size runs two whole passes and 767 or 768 float4s of a third."""
    k = FORMS.index((kind, mom))
    return [Case(kind, mom, WRAP_SIZES[0], (1, 3)[k % 2], 2), Case(kind, mom, WRAP_SIZES[1], (3, 1)[k % 2], 1000)]


def head_of(case):
    """Elements before the first 16-byte boundary (the kernels' scalar head), and the float4 count of the body."""
    head = min((4 - case.mis) % 4, case.n)
    return head, (case.n - head) // 4


def f32(x):
    return float(np.float32(x))


def row(kind, mom, step, lr=LR):
    """The seven scalars as Python floats (doubles): lr, a, b, eps, weight decay, c1, c2.  Every hyper-parameter is the
    fp32 value the C entry receives; the bias corrections are raised in double from those, as jspsr_optim_step, jspsr_adamw_step
    and torch do (they are rounded to fp32 only where the row is handed to `step64` / `step32` / the kernel)."""
    if kind == SGD:
        return [f32(lr), SGD_MOMENTUM if mom else 0.0, 0.0, 0.0, SGD_WD, 1.0 if step == 1 else 0.0, 0.0]
    if kind == RMSPROP:
        return [f32(lr), f32(RMS_MOMENTUM) if mom else 0.0, f32(ALPHA), f32(RMS_EPS), f32(WD), 0.0, 0.0]
    b1, b2 = f32(BETAS[0]), f32(BETAS[1])
    return [f32(lr), b1, b2, f32(ADAM_EPS), f32(WD), 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5]


def _folded(rs, n, lo, hi):
    x = rs.standard_normal(n)
    return (np.where(x < 0, -1.0, 1.0) * np.clip(np.abs(x), lo, hi)).astype(np.float32)


def _seed(case):
    return [case.kind, int(case.mom), case.n % (2 ** 31), case.mis, case.step]


def operands(case):
    """P, G, S1, S2 as fp32 arrays of n elements (all four always: a buffer the form does not own must come back unchanged)."""
    rs = np.random.RandomState(_seed(case))
    n = case.n
    if case.kind == SGD:
        odd = lambda: (2 * rs.randint(-32, 32, n) + 1).astype(np.float32)
        return odd(), rs.randint(-16, 17, n).astype(np.float32), odd(), odd()
    P, G = _folded(rs, n, 0.25, 4.0), _folded(rs, n, 0.25, 2.0)
    first, second = _folded(rs, n, 0.5, 4.0), np.abs(_folded(rs, n, 0.25, 1.0)) ** 2
    return (P, G, first, second) if case.kind in (ADAM, ADAMW) else (P, G, second, first)


def _step(dt, kind, mom, P, G, S1, S2, r):
    """One update in dtype `dt`; every operation is a numpy operation on arrays or scalars of `dt`, so each rounds once."""
    lr, a, b, eps, wd, c1, c2 = (dt(x) for x in r)
    one = dt(1)
    P, G = P.astype(dt), G.astype(dt)
    S1 = None if S1 is None else S1.astype(dt)
    S2 = None if S2 is None else S2.astype(dt)
    if kind == ADAMW:
        P = P * (one - lr * wd)                      # decoupled decay
    else:
        G = G + wd * P                               # coupled: L2 added to the gradient
    if kind == SGD:
        if mom:
            S1 = G if c1 != 0 else a * S1 + G        # the first step's buffer IS the gradient; dampening 0
            G = S1
        P = P - lr * G
    elif kind == RMSPROP:
        S1 = b * S1 + (one - b) * G * G
        q = G / (np.sqrt(S1) + eps)                  # eps outside the root
        if mom:
            S2 = a * S2 + q
            P = P - lr * S2
        else:
            P = P - lr * q
    else:
        S1 = a * S1 + (one - a) * G
        S2 = b * S2 + (one - b) * G * G
        P = P - (lr / c1) * S1 / (np.sqrt(S2) / c2 + eps)
    return P, S1, S2


def step64(kind, mom, P, G, S1, S2, r, round_row=True):
    """(P, S1, S2) after one update, float64.  round_row=False keeps the row's doubles: only the comparison with torch.optim
    uses it, because torch holds the bias corrections in double while the kernel receives their fp32 roundings."""
    r = [f32(x) for x in r] if round_row else list(r)
    u1, u2 = owns(kind, mom)
    out = _step(np.float64, kind, mom, P, G, S1 if u1 else None, S2 if u2 else None, r)
    return out[0], (out[1] if u1 else None), (out[2] if u2 else None)


def step32(kind, mom, P, G, S1, S2, r):
    u1, u2 = owns(kind, mom)
    out = _step(np.float32, kind, mom, P, G, S1 if u1 else None, S2 if u2 else None, [f32(x) for x in r])
    return out[0], (out[1] if u1 else None), (out[2] if u2 else None)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


Result = namedtuple("Result", "ops ref ref32 d bound exact")


def evaluate(case):
    """Operands, the fp64 reference, step32, d = max|step32 - step64| per buffer and the GPU bound 4 d + ulp32(max|ref|) per
    buffer (None for a buffer the form does not own); exact: the reference equals its own fp32 rounding and step32."""
    ops = operands(case)
    r = row(case.kind, case.mom, case.step)
    ref = step64(case.kind, case.mom, *ops, r)
    ref32 = step32(case.kind, case.mom, *ops, r)
    d, bound, exact = [], [], True
    for a, b in zip(ref, ref32):
        if a is None:
            d.append(None), bound.append(None)
            continue
        d.append(float(np.abs(b.astype(np.float64) - a).max()))
        bound.append(4.0 * d[-1] + ulp32(np.abs(a).max()))
        exact = exact and np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.array_equal(b.astype(np.float64), a)
    return Result(ops, ref, ref32, d, bound, exact)


@functools.lru_cache(maxsize=None)
def evaluate_small(case):
    return evaluate(case)


# ---- planted mistakes -------------------------------------------------------------------------------------------------
MISTAKES = ("head_skipped", "head_twice", "left_gradient", "pass_skipped", "stale_row")


def applies(name, case):
    head, n4 = head_of(case)
    if name in ("head_skipped", "head_twice"):
        return head > 0
    if name == "left_gradient":
        return n4 > 0 and case.n > 1
    if name == "pass_skipped":
        return 4 * n4 > GRID
    # A stale row is the row of step - 1.  It is a planted case where that row differs by far more than the rounding: at
    # step 2 (SGD with momentum: the first-step flag; Adam, AdamW: c1 0.1 for 0.19).  At step 1000 the two rows differ by
    # 2e-4 relative in c2 alone, at ADAM_LATE not in a single bit, and the other forms' rows do not depend on the step.
    return case.step == 2 and (case.kind in (ADAM, ADAMW) or (case.kind == SGD and case.mom))


def _put(dst, src, sl):
    out = []
    for a, b in zip(dst, src):
        if a is None:
            out.append(None)
        else:
            a = a.copy()
            a[sl] = b[sl]
            out.append(a)
    return tuple(out)


def planted(name, case, res):
    """The reference's output (P, S1, S2) with mistake `name` planted in it."""
    kind, mom = case.kind, case.mom
    P, G, S1, S2 = res.ops
    r = row(kind, mom, case.step)
    head, n4 = head_of(case)
    start = (P.astype(np.float64), S1.astype(np.float64), S2.astype(np.float64))
    if name == "head_skipped":                           # element 0 keeps what it held
        return _put(res.ref, start, slice(0, 1))
    if name == "head_twice":                             # element 0 goes through the update again
        one = slice(0, 1)
        again = _step(np.float64, kind, mom, res.ref[0][one], G[one], *(None if b is None else b[one] for b in res.ref[1:]),
                      [f32(x) for x in r])
        return tuple(None if a is None else np.concatenate((b, a[1:])) for a, b in zip(res.ref, again))
    if name == "left_gradient":                          # one body element reads its left neighbour's gradient
        lo = max(head, 1)
        hi = min(head + 4 * n4, lo + 4096)
        i = lo + int(np.argmax(np.abs(G[lo:hi].astype(np.float64) - G[lo - 1:hi - 1])))
        one = slice(i, i + 1)
        wrong = step64(kind, mom, P[one], G[i - 1:i], S1[one], S2[one], r)
        return tuple(None if a is None else np.concatenate((a[:i], b, a[i + 1:])) for a, b in zip(res.ref, wrong))
    if name == "pass_skipped":                           # the second trip of the grid-stride loop never happens
        return _put(res.ref, start, slice(head + GRID, min(head + 2 * GRID, head + 4 * n4)))
    if name == "stale_row":
        return step64(kind, mom, P, G, S1, S2, row(kind, mom, case.step - 1))
    raise ValueError(name)


def margin(case, res, mutant):
    """How far the mutant stands from the reference, in units of the GPU bound: (the largest ratio over the buffers -- a test
    fails as soon as one buffer leaves its bound --, the ratio of the parameters alone).  For an exact case: inf where an
    fp32 bit differs, else 0."""
    ratios = []
    for a, m, b in zip(res.ref, mutant, res.bound):
        if a is None:
            continue
        if res.exact:
            ratios.append(0.0 if np.array_equal(a.astype(np.float32), m.astype(np.float32)) else float("inf"))
        else:
            ratios.append(float(np.abs(m - a).max()) / b)
    return max(ratios), ratios[0]
