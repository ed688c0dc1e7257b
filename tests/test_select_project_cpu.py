"""CPU: the fused Selection + Projection handle (tsq_project_*, ABI 10) is declared, bound and exported, and its constructor
refuses a NULL context without touching *out."""
import ctypes as C

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E

NAMES = ["tsq_project_create", "tsq_project_run", "tsq_project_set_jit", "tsq_project_str_warnings", "tsq_project_stats", "tsq_project_destroy"]


def test_project_symbols_are_bound_and_exported():
    lib = _lib.load()
    for name in NAMES:
        assert name in abi.SIGNATURES, name
        assert hasattr(lib, name), "libtsq.so does not export %s" % name


def test_abi_version_is_10():
    assert abi.TSQ_ABI_VERSION == 10
    assert _lib.load().tsq_abi_version() == 10


def test_project_create_with_a_null_context_is_invalid_and_leaves_out_alone():
    lib = _lib.load()
    progs = E.compile_list([E.ScalarFunction("plus", E.Column(0, abi.I64), E.Constant(1))])
    out = C.c_void_p(0x1234)
    assert lib.tsq_project_create(None, None, 0, progs, 1, C.byref(out)) == abi.ERR_INVALID
    assert out.value == 0x1234
