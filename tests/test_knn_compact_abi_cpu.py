"""The compaction entry points of the C ABI (include/mrag.h, K15) on a machine without a GPU:
exported, bound in app._native, and rejecting bad arguments before any HIP call."""
from __future__ import annotations

import ctypes

import pytest

SYMBOLS = ("mrag_knn_live_rows", "mrag_knn_compact", "mrag_knn_row_remap")


@pytest.fixture(scope="module")
def lib():
    from app import _native

    return _native.load()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_and_bound(lib, name):
    from app import _native

    assert hasattr(lib, name)
    assert name in _native.SIGNATURES


def test_compact_null_index_is_an_argument_error(lib):
    size = ctypes.c_int64(-7)
    rc = lib.mrag_knn_compact(None, None, ctypes.byref(size))
    assert rc == 1
    assert b"NULL" in lib.mrag_last_error()
    assert size.value == -7  # nothing written


def test_live_rows_null_arguments(lib):
    n = ctypes.c_int64(0)
    assert lib.mrag_knn_live_rows(None, ctypes.byref(n)) == 1
    assert b"NULL" in lib.mrag_last_error()


def test_row_remap_bad_arguments(lib):
    live = ctypes.c_int64(-1)
    assert lib.mrag_knn_row_remap(None, -1, None, ctypes.byref(live), None) == 1
    assert b"out of range" in lib.mrag_last_error()
    assert lib.mrag_knn_row_remap(None, 1 << 31, None, ctypes.byref(live), None) == 1
    assert lib.mrag_knn_row_remap(None, 8, None, ctypes.byref(live), None) == 1  # NULL device pointers
    assert b"NULL" in lib.mrag_last_error()
    assert lib.mrag_knn_row_remap(None, 8, None, None, None) == 1
    # pointers that are not 16-byte aligned are refused before they are used
    assert lib.mrag_knn_row_remap(ctypes.c_void_p(4), 8, ctypes.c_void_p(32), ctypes.byref(live), None) == 1
    assert b"aligned" in lib.mrag_last_error()
    # n = 0 needs no device: nothing to do
    assert lib.mrag_knn_row_remap(None, 0, None, ctypes.byref(live), None) == 0
    assert live.value == 0
