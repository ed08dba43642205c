"""Completeness of the LDS poison tier (CPU): every ``ncnet_*`` launcher declared
in csrc/launchers.h whose defining .hip file uses ``__shared__`` has a case in
tests/lds_poison_cases.py or an entry with a reason in its EXEMPT dict, so a new
LDS kernel without a poison case fails here."""
import re
from pathlib import Path

from tests import lds_poison_cases as LP

CSRC = Path(__file__).resolve().parent.parent / "ncnet_amd" / "csrc"


def _declared():
    return set(re.findall(r"^\s*int\s+(ncnet_\w+)\s*\(", (CSRC / "launchers.h").read_text(), re.M))


def _defined_in_lds_files():
    """launcher -> source file, for the sources that declare any LDS"""
    out = {}
    for src in sorted(CSRC.glob("*.hip")):
        text = src.read_text()
        if "__shared__" not in text:
            continue
        for name in re.findall(r'^extern "C" int (ncnet_\w+)\s*\(', text, re.M):
            out[name] = src.name
    return out


def test_every_lds_launcher_has_a_case_or_an_exemption():
    declared, lds = _declared(), _defined_in_lds_files()
    assert len(declared) > 50 and len(lds) > 40            # the regexes still find the launchers
    assert set(lds) <= declared, sorted(set(lds) - declared)
    covered = {name for c in LP.CASES for name in c.launchers}
    missing = sorted(n for n in lds if n not in covered and n not in LP.EXEMPT)
    assert not missing, f"LDS launchers without a poison case or an exemption: {[(n, lds[n]) for n in missing]}"


def test_case_table_is_consistent():
    declared, lds = _declared(), _defined_in_lds_files()
    ids = [c.id for c in LP.CASES]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    for c in LP.CASES:
        assert c.launchers, c.id
        for name in c.launchers:
            assert name in declared and name in lds, (c.id, name)
    covered = {name for c in LP.CASES for name in c.launchers}
    for name, reason in LP.EXEMPT.items():
        assert name in declared, f"exempt launcher {name} is not declared in launchers.h"
        assert isinstance(reason, str) and len(reason.strip()) >= 10, f"{name}: an exemption needs a reason"
        assert name not in covered, f"{name} is exempt and has a case"
    # the three patterns of the tier: zeros, NaN in every staged format, fp32 -inf
    assert dict(LP.PATTERNS) == {"zeros": 0x00000000, "nan": 0x7FC07FC0, "neginf": 0xFF800000}
