"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/g14_infer.npz: the numbers the reference's own whole-scene helpers
produce (utils/utils.py add_padding / remove_padding / cal_pad, :1501-1553; data/data_utils.py ToTensor.scale_data,
:289-312) on the frozen inputs of tests/infer_ref.py.

`utils.utils` imports half of the reference's dependencies at module level.  Only four pure numpy functions are wanted,
so their definitions are taken out of the files' syntax trees at generation time and compiled on their own, with numpy
and torch as their only globals.  None of the reference's text is kept: the fixture holds arrays only.

Run where the reference tree is available (never on the GPU box):

    python tools/gen_golden_infer.py

 pad{i}            add_padding of PAD_CASES[i]                      unpad{i}   remove_padding of pad{i}
 cal_pad           cal_pad of an (s, s, 1) array for s in CAL_PAD_SIDES
 scale_{log|lin}_{base|nobase}   scale_data of the 40 x 40 DEM after add_padding(., DEM_PAD), min -80, max 933
"""
from __future__ import annotations

import ast
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402
from tests import infer_ref as R  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g14_infer.npz")


def _compile(path, names, inside=None):
    """The function definitions `names` of the file (of class `inside`, if given), compiled alone."""
    tree = ast.parse(open(path).read(), path)
    body = tree.body
    if inside is not None:
        body = [n for n in body if isinstance(n, ast.ClassDef) and n.name == inside][0].body
    found = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in found) == sorted(names), (path, names)
    for n in found:
        n.decorator_list = []                       # staticmethod: called as a plain function here
    ns = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=found, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def reference_available(ref=G.REF) -> bool:
    return os.path.isfile(os.path.join(ref, "utils", "utils.py")) and os.path.isfile(os.path.join(ref, "data", "data_utils.py"))


def generate(ref=G.REF) -> dict:
    add_padding, remove_padding, cal_pad = _compile(os.path.join(ref, "utils", "utils.py"), ["add_padding", "remove_padding", "cal_pad"])
    (scale_data,) = _compile(os.path.join(ref, "data", "data_utils.py"), ["scale_data"], inside="ToTensor")
    arrays, dem = R.golden_inputs()
    store = {"seed": np.int64(R.SEED), "inputs_checksum": np.array(R.inputs_checksum())}
    for i, (a, (_, _, _, n)) in enumerate(zip(arrays, R.PAD_CASES)):
        store[f"pad{i}"] = add_padding(a, n)
        store[f"unpad{i}"] = np.ascontiguousarray(remove_padding(store[f"pad{i}"], n))
    store["cal_pad"] = np.array([cal_pad(np.zeros((s, s, 1), np.float32)) for s in R.CAL_PAD_SIDES], dtype=np.int64)
    padded = add_padding(dem, R.DEM_PAD)
    base = float(np.min(dem))
    for log in (True, False):
        for with_base in (True, False):
            store[f"scale_{'log' if log else 'lin'}_{'base' if with_base else 'nobase'}"] = scale_data(
                padded, R.ELEV_MIN, R.ELEV_MAX, log, base_elev=base if with_base else 0.0)
    return store


def main():
    store = generate()
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
