"""mvsdet_amd.ops is a package of one module per stage; what `ops.<name>` resolves to is what the single module resolved to.

tests/golden/ops_surface.json was written by tests/golden/make_ops_surface.py on the commit before the split: every public
name with its schema / signature / fields / value, the members of the AUTOCAST_FP32_* tuples, and what the sweep family's fake
kernels return.  The same function recomputes it here.  No GPU: the fakes that size a table call a host-only function of the library.
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

RETIRED = {"get_option"}   # duplicated _lib.get_option and had no caller


@pytest.fixture(scope="module")
def surfaces():
    spec = importlib.util.spec_from_file_location("make_ops_surface", os.path.join(GOLDEN, "make_ops_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "ops_surface.json")) as fh:
        want = json.load(fh)
    return want, json.loads(json.dumps(mod.surface()))


def test_public_names_are_the_parents(surfaces):
    want, got = surfaces
    assert set(want["names"]) - set(got["names"]) == RETIRED
    assert set(got["names"]) - set(want["names"]) == set()
    for name, entry in want["names"].items():
        if name not in RETIRED:
            assert got["names"][name] == entry, name


def test_autocast_tuples_hold_the_same_operators(surfaces):
    want, got = surfaces
    assert got["autocast"] == want["autocast"]


def test_sweep_fakes_return_the_same_shapes_and_dtypes(surfaces):
    want, got = surfaces
    assert got["sweep_fakes"] == want["sweep_fakes"]


def test_every_custom_op_is_registered_once(surfaces):
    import torch
    from mvsdet_amd import ops
    want, _ = surfaces
    names = [n for n, e in want["names"].items() if e["kind"] == "op"]
    assert len(names) == 37
    for n in names:
        overload = getattr(torch.ops.mvsdet_amd, n).default          # raises if the operator was never registered
        assert getattr(ops, n)._opoverload is overload, n            # ... and ops.<name> is that one registration
