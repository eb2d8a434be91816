"""The window count on 2-bit packed sequences without a GPU: the four calls are declared, bound and exported and refuse
a NULL handle before anything touches a device."""
import ctypes as C
import os

import numpy as np
import pytest

from fm_index_amd import _lib

CALLS = {"fmx_count_windows_packed2_dev": 10, "fmx_count_windows_packed2": 8,
         "fmx_count_windows_packed2_rc_dev": 10, "fmx_count_windows_packed2_rc": 8}


@pytest.mark.parametrize("name", list(CALLS))
def test_entry_point_is_declared_bound_exported_and_refuses_null(name):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmx.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    assert "int %s(" % name in header and name in bound and len(bound[name][2]) == CALLS[name]
    off = np.array([0, 2], dtype=np.uint64)
    mid = (2, 1) if name.endswith("_dev") else (1,)                 # (total_syms,) k
    args = (None, None, off.ctypes.data_as(C.c_void_p), 1) + mid
    assert getattr(_lib.lib(), name)(*(args + (None,) * (CALLS[name] - len(args)))) == _lib.ERR_ARG
