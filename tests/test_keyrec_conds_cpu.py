"""The boundary of OtherConditions on the key-record route: knob TSQ_KNOB_KEYREC_CONDS = 42 in the header and in the Python ABI
mirror; the knob table keeps its size (no struct changed: the ABI version stays what it was)."""
import os
import re

from tinysql_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_knobs():
    text = open(os.path.join(ROOT, "include", "tsq.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(?m)^\s+TSQ_KNOB_(\w+) = (\d+)", text)}  # (the enumerators, not the comments that speak of them)


def test_header_names_the_knob():
    knobs = _header_knobs()
    assert knobs["KEYREC_CONDS"] == 42
    assert knobs["COUNT"] == 48
    assert sorted(v for k, v in knobs.items() if k != "COUNT") == list(range(43))  # dense, no number twice


def test_python_mirror_names_the_knob():
    assert abi.KNOB_KEYREC_CONDS == 42
    knobs = _header_knobs()
    for name, value in knobs.items():
        if name != "COUNT":
            assert getattr(abi, "KNOB_" + name) == value, name
