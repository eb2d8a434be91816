"""2-bit packed patterns without a GPU: the three calls are declared, bound and exported and refuse a NULL handle before
anything touches a device; pack2 writes the layout of include/fmx.h (hand-worked)."""
import ctypes as C
import os

import numpy as np

import fm_index_amd as F
from fm_index_amd import _lib


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmx.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for nm in ("fmx_count_batch_packed2_dev", "fmx_count_batch_packed2", "fmx_packed2_supported"):
        assert "int %s(" % nm in header and nm in bound
    assert [len(bound[n][2]) for n in ("fmx_count_batch_packed2_dev", "fmx_count_batch_packed2",
                                       "fmx_packed2_supported")] == [9, 8, 1]
    lib = _lib.lib()
    off = np.zeros(2, dtype=np.uint64)
    po = off.ctypes.data_as(C.c_void_p)
    assert lib.fmx_count_batch_packed2(None, None, po, 1, None, None, None, None) == _lib.ERR_ARG
    assert lib.fmx_count_batch_packed2_dev(None, None, po, 1, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.fmx_packed2_supported(None) == 0


def test_pack2_layout_by_hand():
    """[1, 2, 3, 4] at symbols 30..33: codes 0 and 1 in the top four bits of word 0, codes 2 and 3 in the low four bits
    of word 1; the 30 symbols in front belong to nobody and leave no bits"""
    flat = np.array([4] * 30 + [1, 2, 3, 4], dtype=np.uint8)
    words, off = F.pack2(flat=flat, off=np.array([30, 34], dtype=np.uint64))
    assert words.dtype == np.uint64 and off.tolist() == [30, 34]
    assert words.tolist() == [1 << 62, 2 | 3 << 2]
    words, off = F.pack2([b"\x01\x02", b"", b"\x04"])
    assert off.tolist() == [0, 2, 2, 3] and words.tolist() == [0 | 1 << 2 | 3 << 4]
