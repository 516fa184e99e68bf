"""The optimizer kernels' yardstick, checked without a GPU (tests/optim_step_ref.py):

* `step64` IS torch.optim: SGD, Adam, AdamW and RMSprop in float64, every form, weight decay on and off, after 1 and after 3
  chained steps, parameters and every state buffer, to 1e-13 of the buffer's largest magnitude.  torch keeps Adam's bias
  corrections in double while the kernels receive their fp32 roundings, so this comparison -- and only this one -- hands
  `step64` the row unrounded; a second assertion holds the rounded row to within the rounding of c1 and c2 of it.
* the SGD operands make the arithmetic exact: the fp64 result is an fp32 number and `step32` equals it, on 100 % of the
  elements of every SGD case -- what lets the GPU test ask for bit equality.
* for the other kinds d = max|step32 - step64| per case and buffer gives the GPU bound 4 d + ulp32(max|ref|); every planted
  mistake stands at least 100 x that bound away on every case it applies to (and breaks bit equality on the SGD cases).
"""
import numpy as np
import pytest
import torch

from tests import optim_step_ref as X

FORM_IDS = [X.form_name(*f) for f in X.FORMS]
TORCH = {X.SGD: torch.optim.SGD, X.ADAM: torch.optim.Adam, X.ADAMW: torch.optim.AdamW, X.RMSPROP: torch.optim.RMSprop}
STATE = {X.SGD: ("momentum_buffer", None), X.ADAM: ("exp_avg", "exp_avg_sq"), X.ADAMW: ("exp_avg", "exp_avg_sq"),
         X.RMSPROP: ("square_avg", "momentum_buffer")}


def torch_kwargs(kind, r):
    if kind == X.SGD:
        return {"lr": r[0], "momentum": r[1], "weight_decay": r[4]}
    if kind == X.RMSPROP:
        return {"lr": r[0], "momentum": r[1], "alpha": r[2], "eps": r[3], "weight_decay": r[4]}
    return {"lr": r[0], "betas": (r[1], r[2]), "eps": r[3], "weight_decay": r[4]}


@pytest.mark.parametrize("decay", [True, False], ids=["wd", "nowd"])
@pytest.mark.parametrize("kind,mom", X.FORMS, ids=FORM_IDS)
def test_step64_is_torch_optim(kind, mom, decay):
    n = 257
    rs = np.random.RandomState(100 + 2 * X.FORMS.index((kind, mom)) + decay)
    start = rs.standard_normal(n)
    grads = [rs.standard_normal(n) for _ in range(3)]
    rows = [X.row(kind, mom, t) for t in (1, 2, 3)]
    if not decay:
        for r in rows:
            r[4] = 0.0
    p = torch.nn.Parameter(torch.from_numpy(start.copy()))
    opt = TORCH[kind]([p], **torch_kwargs(kind, rows[0]))
    u1, u2 = X.owns(kind, mom)
    P, S1, S2 = start, np.zeros(n), np.zeros(n)
    for t in range(3):
        p.grad = torch.from_numpy(grads[t].copy())
        opt.step()
        exact = X.step64(kind, mom, P, grads[t], S1, S2, rows[t], round_row=False)
        rounded = X.step64(kind, mom, P, grads[t], S1, S2, rows[t])
        P, S1, S2 = exact[0], exact[1] if u1 else S1, exact[2] if u2 else S2
        if t == 1:
            continue
        want = [p.detach().numpy()] + [None if key is None or not own else opt.state[p][key].numpy()
                                       for key, own in zip(STATE[kind], (u1, u2))]
        for name, got, ref, rnd in zip(("P", "S1", "S2"), exact, want, rounded):
            assert (got is None) == (ref is None), (name, t)
            if got is None:
                continue
            scale = np.abs(ref).max()
            err = np.abs(got - ref).max()
            print(f"{X.form_name(kind, mom)} wd={decay} step {t + 1} {name}: |step64 - torch| {err:.2e} of {scale:.2e}")
            assert err <= 1e-13 * scale, (name, t, err, scale)
            # the row as the kernel receives it: c1 and c2 each within 2^-24 relative, and they only scale the update
            assert np.abs(rnd - got).max() <= 2.0 ** -22 * np.abs(P - start).max() + 1e-300, (name, t)
    assert not u1 or STATE[kind][0] in opt.state[p]
    assert u2 or STATE[kind][1] is None or STATE[kind][1] not in opt.state[p]      # torch makes no buffer this form lacks


def test_rows_hold_what_the_header_documents():
    assert X.row(X.SGD, True, 1)[5] == 1.0 and X.row(X.SGD, True, 2)[5] == 0.0
    r1, r2, late = X.row(X.ADAM, True, 1), X.row(X.ADAMW, True, 2), X.row(X.ADAM, True, X.ADAM_LATE)
    assert abs(r1[5] - 0.1) < 1e-7 and abs(r2[5] - 0.19) < 1e-7 and late[5] == 1.0 and 0.0 < late[6] < 1.0
    assert X.f32(late[1]) ** X.ADAM_LATE == 0.0                 # beta1^t has underflowed
    for kind, mom in X.FORMS:
        for step in X.steps_of(kind):
            assert len(X.row(kind, mom, step)) == 7
    # the geometry: every head length, bodies of 0, 1 and many float4s, tails of 0..3, and both wrap sizes past one pass
    seen = {(X.head_of(c)[0], min(X.head_of(c)[1], 2), c.n - X.head_of(c)[0] - 4 * X.head_of(c)[1]) for c in X.small_cases(X.SGD, False)}
    assert {h for h, _, _ in seen} == {0, 1, 2, 3} and {b for _, b, _ in seen} == {0, 1, 2} and {t for _, _, t in seen} == {0, 1, 2, 3}
    for kind, mom in X.FORMS:
        a, b = X.wrap_cases(kind, mom)
        # the first size fills one pass to the last float4 (head 3) or starts the second with a single float4 (head 1);
        # the second size runs two whole passes and part of a third
        assert 4 * X.head_of(a)[1] == X.GRID + (4 if a.mis == 3 else 0) and 2 * X.GRID < 4 * X.head_of(b)[1] < 3 * X.GRID
        assert {a.mis, b.mis} == {1, 3}


@pytest.mark.parametrize("mom", [False, True], ids=["plain", "momentum"])
def test_sgd_operands_make_the_update_exact(mom):
    for case in X.small_cases(X.SGD, mom):                      # (the wrap-sized cases: asserted with their planted mistakes below)
        res = X.evaluate_small(case)
        assert res.exact, case                                  # 100 % of the elements, P and the momentum buffer
        assert all(d is None or d == 0.0 for d in res.d), case
        P, G, S1, _ = res.ops
        assert np.abs(P).max() <= 64 and np.abs(S1).max() <= 64 and np.abs(G).max() <= 16
        assert np.array_equal(P, np.round(P)) and np.array_equal(G, np.round(G)) and np.array_equal(S1, np.round(S1))


@pytest.mark.parametrize("kind,mom", X.FORMS, ids=FORM_IDS)
def test_planted_mistakes_stand_100_bounds_away(kind, mom):
    worst_d = [0.0, 0.0, 0.0]
    margins = {m: float("inf") for m in X.MISTAKES}             # over the buffers: what fails a test
    margins_p = {m: float("inf") for m in X.MISTAKES}           # the parameters alone
    hits = {m: 0 for m in X.MISTAKES}
    for case in X.small_cases(kind, mom) + X.wrap_cases(kind, mom):
        res = X.evaluate_small(case) if case.n < X.GRID else X.evaluate(case)
        assert res.exact == (kind == X.SGD), case
        for k, d in enumerate(res.d):
            assert (d is None) == (not ((True,) + X.owns(kind, mom))[k])
            if d is not None:
                worst_d[k] = max(worst_d[k], d)
        if kind != X.SGD:
            assert np.abs(res.ops[0]).max() <= 4.0
        for m in X.MISTAKES:
            if not X.applies(m, case):
                continue
            hits[m] += 1
            got, got_p = X.margin(case, res, X.planted(m, case, res))
            margins[m], margins_p[m] = min(margins[m], got), min(margins_p[m], got_p)
            assert got >= 100.0 and got_p >= 100.0, (m, case, got, got_p, res.bound)
    print(f"{X.form_name(kind, mom)}: d = max|step32 - step64| over the cases: P {worst_d[0]:.3e}  S1 {worst_d[1]:.3e}  S2 {worst_d[2]:.3e}")
    print(f"{X.form_name(kind, mom)}: smallest margin (x bound) " + "  ".join(f"{m} {margins[m]:.3g} / P alone {margins_p[m]:.3g} ({hits[m]} cases)" for m in X.MISTAKES))
    stale = kind in (X.ADAM, X.ADAMW) or (kind == X.SGD and mom)
    assert all(hits[m] > 0 for m in X.MISTAKES if m != "stale_row") and (hits["stale_row"] > 0) == stale
