"""TSQ_KNOB_JOIN_BATCH_TIMING is id 44 of the knob table in the header and in the Python mirror; the table keeps its size and the ABI
version its value (no struct changed)."""
import os
import re

from tinysql_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_mirror_name_the_knob():
    text = open(os.path.join(ROOT, "include", "tsq.h")).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"(?m)^#define TSQ_KNOB_(\w+) (\d+)\s*$", text)}
    assert defines["JOIN_BATCH_TIMING"] == 44 == abi.KNOB_JOIN_BATCH_TIMING
    assert len(set(defines.values())) == len(defines)  # no id twice among the ids behind the enumerators
    count = int(re.search(r"(?m)^\s+TSQ_KNOB_COUNT = (\d+)", text).group(1))
    assert count == 48 and all(43 <= v < count for v in defines.values())
    assert int(re.search(r"(?m)^#define TSQ_ABI_VERSION (\d+)", text).group(1)) == 10
