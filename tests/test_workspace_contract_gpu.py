"""GPU: every case of tests/workspace_cases.py in guarded arenas.  Each buffer of a call -- inputs, outputs, workspace -- is
a 4096-byte front guard, the payload and a 4096-byte back guard, all of byte 0xA5; the payload starts on a 256-byte
boundary and the workspace payload is exactly the bytes its query returned, so its back guard begins at an unrounded
offset.  A case runs three times: (a) a roomy zeroed workspace and zeroed outputs, (b) the exact workspace and the
outputs filled with 0xA5, (c) the same filled with 0x00.  An overrun shows as a damaged guard, a read of something never
written as a difference between the three runs, an output element left out as a surviving 0xA5 pattern.  The highest
workspace byte written in (b) is held to the table's touched_bytes, which the CPU file carries to large shapes.  A
workspace 4 bytes off and the arguments at each documented refusal boundary are refused with an unchanged census; the
propagation cases run once more in a child process per JSPSR_PROP_* setting ("What the workspace contract pins")."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import workspace_cases as WC

pytestmark = pytest.mark.gpu

GUARD, PATTERN, ROOMY = 4096, 0xA5, 1 << 20


def _lib():
    from jspsr_amd import _lib
    return _lib.load()


def _census(lib):
    return {n: lib.jspsr_launch_count(n.encode()) for n in WC.ALL_LAUNCHES}


class Arena:
    def __init__(self, nbytes, fill):
        self.n = nbytes
        self.whole = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device="cuda")
        self.whole.fill_(PATTERN)
        self.payload = self.whole[GUARD:GUARD + nbytes]
        if fill is not None and nbytes:
            self.payload.fill_(fill)
        assert (self.whole.data_ptr() + GUARD) % 256 == 0, "payload not on a 256-byte boundary"

    @property
    def ptr(self):
        return self.whole.data_ptr() + GUARD

    def load(self, arr):
        src = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy())
        assert src.numel() == self.n
        if self.n:
            self.payload.copy_(src)

    def guards_intact(self):
        return bool((self.whole[:GUARD] == PATTERN).all()) and bool((self.whole[GUARD + self.n:] == PATTERN).all())


class Ctx:
    """mode: 'roomy' (a), 'a5' (b), 'zero' (c); expect: the return code every call must give; ws_shift: bytes added to
    the workspace pointer (4 only where a refusal is expected: nothing misaligned is ever launched)."""

    def __init__(self, lib, nbytes, mode, expect=0, ws_shift=0):
        self.lib, self.nbytes, self.mode, self.expect, self.ws_shift = lib, nbytes, mode, expect, ws_shift
        self.stream = torch.cuda.current_stream().cuda_stream
        self.arenas, self.outs, self.accs, self.inputs = {}, {}, {}, {}
        fill = {"roomy": 0, "a5": PATTERN, "zero": 0}[mode]
        self.fill = fill
        self.wsa = Arena(nbytes + (ROOMY if mode == "roomy" else 0), fill)
        self.arenas["workspace"] = self.wsa

    def ws(self):
        return self.wsa.ptr + self.ws_shift

    def inp(self, name, arr):
        arr = np.ascontiguousarray(arr)
        a = Arena(arr.nbytes, None)
        a.load(arr)
        self.arenas[name] = a
        self.inputs[name] = arr
        return a.ptr

    def out(self, name, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = Arena(n, self.fill)
        self.arenas[name] = a
        self.outs[name] = (a, np.dtype(dtype).itemsize)
        return a.ptr

    def acc(self, name, arr):
        a = Arena(arr.nbytes, None)
        a.load(arr)
        self.arenas[name] = a
        self.accs[name] = a
        return a.ptr

    def call(self, fn, *args):
        rc = getattr(self.lib, fn)(*args)
        assert rc == self.expect, f"{fn} returned {rc}, expected {self.expect}: {self.lib.jspsr_last_error().decode(errors='replace')}"

    def finish(self, tag):
        torch.cuda.synchronize()
        for name, a in self.arenas.items():
            assert a.guards_intact(), f"{tag}: a guard of `{name}` was written"
        for name, arr in self.inputs.items():
            got = self.arenas[name].payload.cpu().numpy()
            assert np.array_equal(got, arr.reshape(-1).view(np.uint8)), f"{tag}: input `{name}` changed"
        res = {n: a.payload.clone() for n, (a, _) in self.outs.items()}
        res.update({n: a.payload.clone() for n, a in self.accs.items()})
        return res


def _run(lib, name, query, qargs, run, launches, mode):
    nbytes = getattr(lib, query)(*qargs)
    assert nbytes > 0, f"{name}: the query returns 0 for the case's own arguments"
    ctx = Ctx(lib, nbytes, mode)
    before = _census(lib)
    run(ctx)
    res = ctx.finish(f"{name} ({mode})")
    after = _census(lib)
    made = {n: after[n] - before[n] for n in WC.ALL_LAUNCHES}
    assert made == {n: launches.get(n, 0) for n in WC.ALL_LAUNCHES}, f"{name} ({mode}): launched {made}, the case names {launches}"
    return ctx, res, nbytes


def contract(lib, name, query, qargs, run, launches, touched):
    """The three runs of one case and everything asserted about them (module docstring)."""
    args = (lib, name, query, qargs, run, launches)
    _, ra, nbytes = _run(*args, "roomy")
    assert touched <= nbytes, f"{name}: the launches address {touched} bytes, the query promises {nbytes}"
    cb, rb, _ = _run(*args, "a5")
    for out, (a, item) in cb.outs.items():
        stale = (a.payload.view(-1, item) == PATTERN).all(1)
        assert not stale.any(), f"{name}: {int(stale.sum())} elements of `{out}` (documented as overwritten) keep the prefill, " \
                                f"first at {int(stale.nonzero()[0])}"
    written = (cb.wsa.payload != PATTERN).nonzero()
    last = int(written.max()) + 1 if written.numel() else 0
    print(f"{name}: query {nbytes}, touched_bytes {touched}, last byte written {last}")
    assert last > 0 or touched == 0, f"{name}: nothing was written to the workspace"
    assert last <= touched, f"{name}: byte {last - 1} of the workspace was written, touched_bytes says {touched}"
    _, rc, _ = _run(*args, "zero")
    for out in ra:
        assert torch.equal(ra[out], rb[out]), f"{name}: `{out}` depends on what the workspace / outputs held (0xA5 fill)"
        assert torch.equal(ra[out], rc[out]), f"{name}: `{out}` differs between the roomy and the exact workspace"


@pytest.mark.parametrize("case", WC.CASES, ids=[c.name for c in WC.CASES])
def test_workspace_contract(case):
    assert case.bits, "a case without run-to-run bits needs its own comparison"
    contract(_lib(), case.name, case.query, case.qargs, case.run, case.launches, case.touched(*case.qargs))


def run_prop_forms():
    """Child-process entry: the library reads its JSPSR_PROP_* switches once per process.  Every propagation case under the
    setting this process was started with; the query is one function for all forms, so it must cover this one too."""
    env = {k: v for k, v in os.environ.items() if k.startswith("JSPSR_PROP_")}
    lib, n = _lib(), 0
    for name, query, shape, run, entry, kw, _ in WC.prop_cases():
        contract(lib, name, query, shape, run, WC.prop_launches(entry, shape[2], env, **kw), WC.touched_prop(entry, *shape, env))
        n += 1
    torch.cuda.synchronize()
    print(f"contract ok: {n} cases under {env}")


@pytest.mark.parametrize("env", WC.PROP_FORMS, ids=["-".join(f"{k[11:]}{v}" for k, v in e.items()) for e in WC.PROP_FORMS])
def test_prop_switch_forms_in_a_child_process(env):
    """One child per setting of tests/test_prop_gpu.py's list, each under its own time limit; no retry."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from tests.test_workspace_contract_gpu import run_prop_forms; run_prop_forms()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120, cwd=root)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"contract ok: {len(WC.prop_cases())} cases" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


_ALIGNED = [c for c in WC.CASES if c.align == 16]


@pytest.mark.parametrize("case", _ALIGNED, ids=[c.name for c in _ALIGNED])
def test_misaligned_workspace_is_refused(case):
    """Where the header documents 16-byte alignment: a workspace 4 bytes off is JSPSR_EALIGN, and nothing launches."""
    lib = _lib()
    nbytes = getattr(lib, case.query)(*case.qargs)
    ctx = Ctx(lib, nbytes, "roomy", expect=WC.EALIGN, ws_shift=4)
    before = _census(lib)
    case.run(ctx)
    assert _census(lib) == before, f"{case.name}: a launch was made with a misaligned workspace"
    ctx.finish(case.name)


@pytest.mark.parametrize("r", WC.REFUSALS, ids=[r.name for r in WC.REFUSALS])
def test_query_and_entry_agree_at_the_boundary(r):
    lib = _lib()
    q = getattr(lib, r.query)
    assert q(*r.bad) == 0, f"{r.name}: the query accepts {r.bad}"
    ok_bytes = q(*r.ok)
    assert ok_bytes > 0, f"{r.name}: the query refuses {r.ok}"
    ctx = Ctx(lib, ok_bytes, "roomy", expect=r.code)
    before = _census(lib)
    r.run(ctx, r.bad, r.ok)
    assert _census(lib) == before, f"{r.name}: the entry launched with {r.bad}"
    ctx.finish(r.name)
    ctx = Ctx(lib, ok_bytes, "a5")
    r.run(ctx, r.ok, r.ok)
    ctx.finish(r.name + " (inside)")
    after = _census(lib)
    assert {n: after[n] - before[n] for n in WC.ALL_LAUNCHES} == {n: r.launches.get(n, 0) for n in WC.ALL_LAUNCHES}, r.name
