"""No GPU: the case table of tests/workspace_cases.py against the queries themselves (host code of the library).

The table is complete; touched_bytes <= query for every case and for arguments far above the test shapes, where the
Python side is exact integers and a 32-bit wrap inside a query would show; the queries return 0 for the arguments
their header lists as bad."""
import os
import subprocess
import sys

import pytest

from tests import workspace_cases as WC


def _L():
    from jspsr_amd import _lib
    return _lib


def test_table_names_every_query_and_nothing_else():
    """A query added later without a case fails here."""
    L = _L()
    every = sorted(k for k in L.SIGNATURES if k.endswith("_workspace_bytes"))
    lists = [list(WC.HELD), list(WC.ELSEWHERE)]
    named = sorted(n for l in lists for n in l)
    assert len(named) == len(set(named)), "a query is both in HELD and in ELSEWHERE"
    assert named == every, f"missing: {sorted(set(every) - set(named))}, unknown: {sorted(set(named) - set(every))}"
    print(f"{len(every)} queries: {len(WC.HELD)} with cases, {len(WC.ELSEWHERE)} held by an earlier test")
    for q, where in WC.ELSEWHERE.items():
        assert os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), where.split("::")[0])), (q, where)
    assert set(WC.LARGE) == set(WC.HELD) == set(WC.LARGE_TOUCHED), "every held query has its large arguments"
    for c in WC.CASES:
        assert c.launches and c.branch, f"{c.name}: a case names its launches and the branch it takes"
        assert c.align in (2, 4, 16)


@pytest.mark.parametrize("case", WC.CASES, ids=[c.name for c in WC.CASES])
def test_touched_bytes_fit_the_query(case):
    lib = _L().load()
    n = getattr(lib, case.query)(*case.qargs)
    t = case.touched(*case.qargs)
    assert 0 <= t <= n and n > 0, f"{case.name}: touched {t}, query {n}"
    assert t > 0 or "none touched" in case.branch or "nothing touched" in case.branch, f"{case.name}: a case that touches nothing says so"


@pytest.mark.parametrize("query", sorted(WC.LARGE))
def test_touched_bytes_fit_the_query_at_large_arguments(query):
    lib = _L().load()
    for args in WC.LARGE[query]:
        n = getattr(lib, query)(*args)
        t = WC.LARGE_TOUCHED[query](*args)
        assert 0 < t <= n, f"{query}{args}: touched {t}, query {n}"
        assert n - t < 4096 or query in WC.SHARED_MAX, f"{query}{args}: {n - t} bytes of slack: a wrapped product, or a mirror that lost a region"


@pytest.mark.parametrize("query", sorted(WC.ZERO))
def test_queries_return_zero_for_bad_arguments(query):
    lib = _L().load()
    for args in WC.ZERO[query]:
        assert getattr(lib, query)(*args) == 0, f"{query}{args}"


def test_refusal_table_is_consistent_with_the_queries():
    lib = _L().load()
    for r in WC.REFUSALS:
        q = getattr(lib, r.query)
        assert q(*r.bad) == 0 and q(*r.ok) > 0, r.name


def test_prop_query_covers_the_logits_form_under_another_tile_shape():
    """jspsr_prop_backward_workspace_bytes takes a max() over three grids; its third term, the 8 x 64 grid of the logits
    entry's general path, decides only when a lab tile shape (JSPSR_PROP_TH = 16, read once per process) halves the planar
    grid: 2049 x 16 x 3 then gives 2049 planar tiles (the 4096 floor) against 4098 rows of the logits form."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from jspsr_amd import _lib; from tests import workspace_cases as WC; lib = _lib.load(); "
            "n = lib.jspsr_prop_backward_workspace_bytes(2049, 16, 3); t = WC.touched_prop('logits', 2049, 16, 3); "
            "assert t == 16 + 4098 * 40 and t <= n < t + 16, (t, n); print('covered', n)")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, JSPSR_PROP_TH="16"), capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0 and "covered" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
