"""The C++ UnionScanExec of tinysql_amd/host/tsq_host.hpp replaying the reference's dirty-transaction rows on the GPU:
tsq_unionscan_host_test.cpp cites union_scan_test.go row by row, in order, and exits non-zero on any mismatch."""
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tinysql_amd", "host")


@pytest.mark.gpu
def test_dirty_transaction_rows_through_the_cpp_union_scan():
    exe = os.path.join(HOST, "tsq_unionscan_host_test")
    # always through make: a binary built against an older include/tsq.h (struct layouts) must not be run
    subprocess.run(["make", "-C", HOST, "tsq_unionscan_host_test"], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "39 passed, 0 failed" in r.stdout and "PASS :34 order by b, a" in r.stdout


def test_union_scan_host_program_compiles_with_gxx_alone():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", os.path.join(HOST, "tsq_unionscan_host_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
