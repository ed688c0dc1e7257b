"""The C++ IndexLookUpExecutor of tinysql_amd/host/tsq_host.hpp replaying the reference's double-read rows on the GPU:
tsq_lookup_host_test.cpp cites executor_test.go / distsql_test.go case by case, compares the rows in order, and exits non-zero on
any mismatch."""
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tinysql_amd", "host")


@pytest.mark.gpu
def test_double_read_rows_through_the_cpp_index_lookup():
    exe = os.path.join(HOST, "tsq_lookup_host_test")
    # always through make: a binary built against an older include/tsq.h must not be run
    subprocess.run(["make", "-C", HOST, "tsq_lookup_host_test"], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "33 passed, 0 failed" in r.stdout and "PASS :566 keep order, IndexLookupSize = 3 [batch 1024..3]" in r.stdout


def test_lookup_host_program_compiles_with_gxx_alone():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", os.path.join(HOST, "tsq_lookup_host_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
