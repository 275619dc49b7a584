"""CPU-only: the export of the fused kernel's HLL floors.  It is a diagnostic the library exports for the tests
(capi.Ctx.hll_floors), not an entry point of the C ABI: include/krakenuniq_amd.h does not declare it, so neither the symbol
check nor the in-flight contract of tests/test_abi_host.py covers it; here: it is exported, bound, and checks its arguments."""
import ctypes as C
import os
import re

from krakenuniq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_floor_export_is_exported_and_bound_but_not_declared():
    hdr = open(os.path.join(ROOT, "include", "krakenuniq_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "ku_counts_export_floors" not in hdr
    assert "ku_counts_export_floors" not in capi.SIGNATURES
    assert hasattr(capi.lib(), "ku_counts_export_floors")
    assert hasattr(capi.Ctx, "hll_floors")


def test_floor_export_refuses_null_arguments():
    f = capi.lib().ku_counts_export_floors
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]
    assert f(None, None) == -1  # KU_EINVAL
