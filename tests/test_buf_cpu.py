"""The owning types of the host side (tinysql_amd/csrc/tsq_internal.h: DevBuf, PinnedBuf, DevEvent, StreamDrain) without a GPU: the header
is built into a stand-alone sanitized program (tests/buf_main.cpp) that defines the few HIP entry points the header calls over malloc and
counts live blocks.  Every case ends with the block counters and the context's pool and arena accounting where it predicts them; ASan and
UBSan report nothing.  The HIP runtime is not linked and nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["scope_exit", "moves", "foreign", "keep_growth", "vector", "pool_reuse", "arena", "pinned", "early_return", "events", "all"]


def rocm_include():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    root = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    inc = os.path.join(root, "include")
    return inc if os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")) else "/opt/rocm/include"


@pytest.fixture(scope="module")
def buf_out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("buf") / "buf_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", rocm_include(), "-I", os.path.join(ROOT, "include"), "-pthread", os.path.join(ROOT, "tests", "buf_main.cpp"), "-o", str(exe)],
                   check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-600:] + res.stderr[-3000:]
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    return res.stdout.splitlines()


@pytest.mark.parametrize("case", CASES)
def test_owning_types_free_exactly_once(buf_out, case):
    assert "ok " + case in buf_out


def test_the_header_states_its_own_rules():
    """move-only owners (static_assert next to each type) and no non-temporal builtin outside clang"""
    text = open(os.path.join(ROOT, "tinysql_amd", "csrc", "tsq_internal.h")).read()
    for t in ("DevBuf", "PinnedBuf", "DevEvent"):
        assert "static_assert(!std::is_copy_constructible<%s>::value && std::is_nothrow_move_constructible<%s>::value" % (t, t) in text
    assert "defined(__clang__)" in text
