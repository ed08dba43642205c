"""LDS poison tier (run on an MI355X): no kernel's result may depend on what an
earlier kernel left in LDS.

The suite prefills outputs with NaN, which catches elements that were never
written, but it always runs the same kernels in the same order, so whatever a
kernel finds in LDS words it did not write itself is always the same and always
finite.  Here ``lds_poison`` (csrc/lds_poison.hip) fills the whole 160 KiB of
LDS of every CU with a pattern right before each launch of the kernel under
test: zeros, NaN (in every number format the kernels stage) and -inf.  The
outputs under the three patterns must be bit-identical, and the outputs of the
NaN pattern must pass the oracle and bound of the kernel's existing test.

The harness check comes first in the module and gives the sweep its meaning:
``lds_probe`` copies a workgroup's uninitialised LDS out, and every probed
word must be the pattern just written.

Cases: tests/lds_poison_cases.py (also read by the CPU completeness check in
tests/test_lds_poison_cases_cpu.py).
"""
import pytest
import torch

from ncnet_amd.ops import _ext
from tests import lds_poison_cases as LP

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("lds_bytes", [64 * 1024, LP.LDS_ALL])
@pytest.mark.parametrize("name,pattern", LP.PATTERNS, ids=[n for n, _ in LP.PATTERNS])
def test_harness_poison_reaches_the_next_dispatch(name, pattern, lds_bytes):
    """lds_poison then lds_probe on the same stream: 100 % of the probed words hold the pattern, for
    1, CUs / 2 and CUs probing workgroups of 64 KiB and of all 160 KiB."""
    C = _ext.ext()
    want = pattern - (1 << 32) if pattern >= 1 << 31 else pattern          # as int32
    n = lds_bytes // 4
    for G in (1, max(1, _cus() // 2), _cus()):
        out = torch.full((G, n), 0x5A5A5A5A, dtype=torch.int32, device=DEV)    # none of the patterns
        C.lds_poison(pattern, LP.ROUNDS)
        C.lds_probe(out, lds_bytes)
        share = float((out == want).double().mean())
        print(f"lds_probe {name} G={G} lds_bytes={lds_bytes}: {100 * share:.4f} % of the words match")
        assert share == 1.0, f"{name}, G={G}, {lds_bytes} B: only {100 * share:.4f} % of the probed words hold the pattern"


def test_harness_bindings_reject_bad_arguments():
    C = _ext.ext()
    with pytest.raises(RuntimeError):
        C.lds_poison(1 << 32, 1)
    with pytest.raises(RuntimeError):
        C.lds_poison(0, 0)
    with pytest.raises(RuntimeError):
        C.lds_probe(torch.empty((1, 4), dtype=torch.int32), 1024)               # CPU tensor
    with pytest.raises(RuntimeError):
        C.lds_probe(torch.empty((1, 4), dtype=torch.int32, device=DEV), LP.LDS_ALL + 4)
    with pytest.raises(RuntimeError):
        C.lds_probe(torch.empty((1, 1025), dtype=torch.int32, device=DEV), 4096)   # more words than the LDS holds


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("case", LP.CASES, ids=[c.id for c in LP.CASES])
def test_result_does_not_depend_on_lds_contents(case, tune):
    for name, value in case.tuning:
        tune(name, value)
    runs = {}
    for pname, pattern in LP.PATTERNS:
        with LP.poisoned(pattern):
            runs[pname] = case.fn()
    torch.cuda.synchronize()
    base, _ = runs["zeros"]
    for pname in ("nan", "neginf"):
        outs, _ = runs[pname]
        assert outs.keys() == base.keys()
        for k in base:
            same = torch.equal(_bytes(outs[k]), _bytes(base[k]))
            if not same:
                diff = int((_bytes(outs[k]) != _bytes(base[k])).sum())
                nan = int(torch.isnan(outs[k].float()).sum()) if outs[k].is_floating_point() else 0
                pytest.fail(f"{case.id}: output '{k}' differs between LDS filled with zeros and with {pname} "
                            f"({diff} bytes differ, {nan} NaN elements)")
    runs["nan"][1]()                                   # the existing test's oracle and bound, under the NaN pattern
