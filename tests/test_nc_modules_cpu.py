"""The ``ops/nc/`` package behind ``ops/neigh_consensus.py``: every module
imports on its own, the entry module keeps the names the rest of the project
imports from it, and the state that is rebound at run time (``FAST1X``, the
fp8 pin list) is read where it is defined."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ["ncnet_amd.ops.nc", "ncnet_amd.ops.nc.layers", "ncnet_amd.ops.nc.train", "ncnet_amd.ops.nc.x3",
           "ncnet_amd.ops.nc.fp8", "ncnet_amd.ops.nc.fused", "ncnet_amd.ops.neigh_consensus"]


@pytest.mark.parametrize("name", MODULES)
def test_module_imports_alone(name):
    """A fresh interpreter per module: an import cycle shows only when the
    module is the first of the package to be imported."""
    r = subprocess.run([sys.executable, "-c", f"import {name}"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_entry_module_exports():
    nc = importlib.import_module("ncnet_amd.ops.neigh_consensus")
    for name in ("neigh_consensus", "select_path", "layer_kinds", "fast1x_ok", "x3_dropped", "x3_ablation",
                 "neigh_consensus_fused_x2", "neigh_consensus_fused_x2_fp8", "pin_fp8_weights"):
        assert callable(getattr(nc, name)), name


def test_submodules_do_not_import_the_entry_module():
    for name in MODULES[:-1]:
        src = open(importlib.import_module(name).__file__).read()
        assert "neigh_consensus import" not in src and "import neigh_consensus" not in src, name


class _OnGpu:
    """The 25^4 training volume as far as fast1x_ok looks at it."""
    is_cuda = True
    shape = (2, 1, 25, 25, 25, 25)


def test_fast1x_flag_is_read_where_it_is_defined(monkeypatch):
    nc = importlib.import_module("ncnet_amd.ops.neigh_consensus")       # what bench.py imports from
    train = importlib.import_module("ncnet_amd.ops.nc.train")
    args = (["1in", "16", "1out"], [16, 16, 1], [5, 5, 5], _OnGpu(), True)
    assert train.FAST1X is True and not hasattr(nc, "FAST1X")           # one home, no stale copy
    assert nc.fast1x_ok(*args) is True
    monkeypatch.setattr(train, "FAST1X", False)
    assert nc.fast1x_ok(*args) is False
    monkeypatch.setattr(train, "FAST1X", True)
    assert nc.fast1x_ok(*args) is True
    assert nc.fast1x_ok(args[0], args[1], args[2], torch.zeros(_OnGpu.shape[:2] + (1, 1, 1, 1)), True) is False   # CPU tensor


def test_both_fp8_pin_sites_reach_the_collected_list():
    """The layer-wise fp8 weights and the fused e4m3 operands land in the list
    ``pin_fp8_weights().__enter__`` returned (eval/inloc.py PairMatcher keeps
    it for as long as its captured graph lives), nested blocks included."""
    nc = importlib.import_module("ncnet_amd.ops.neigh_consensus")
    fp8 = importlib.import_module("ncnet_amd.ops.nc.fp8")
    fused = importlib.import_module("ncnet_amd.ops.nc.fused")
    torch.manual_seed(0)
    ws = [torch.randn(3, 16, 1, 3, 3, 3) * 0.1, torch.randn(3, 1, 16, 3, 3, 3) * 0.1]
    bs = [torch.rand(16) * 0.1, torch.rand(1) * 0.1]

    def ids(ts):
        return {id(t) for t in ts}

    fp8.pin([torch.zeros(1)])                    # outside a block: dropped
    with nc.pin_fp8_weights() as pins:
        a, b = torch.zeros(1), torch.zeros(2)
        fp8.pin([a])
        fp8.pin((b,))
        assert [id(t) for t in pins] == [id(a), id(b)]
        wq, _ = fp8._fp8_weights_of(ws[0], "1in")                 # the layer-wise site
        tens, _ = fused._fused_weights_f8(ws, bs)                 # the fused e4m3 site
        assert id(wq) in ids(pins) and ids(tens) <= ids(pins)
        with nc.pin_fp8_weights() as inner:
            fused._fused_weights_f8(ws, bs)                       # cache hit: still pinned, in the inner list
            assert ids(tens) <= ids(inner)
        n = len(pins)
        fp8._fp8_weights_of(ws[1], "1out")
        assert len(pins) == n + 1                                 # the outer list is current again
    assert fp8._FP8_PINS is None
