"""Bit-for-bit comparison of float64 results.

np.array_equal compares VALUES: -0.0 == +0.0, so a kernel that seeds a row with its first product, or stores -0.0 for
an empty row, passes it while the serial oracle (every row starts at +0.0) says otherwise.  The serial-order contract is
about bits, so the suite compares the uint64 patterns."""
import numpy as np


def differing_rows(y, y_ref):
    """indices where the two float64 vectors differ in their bit patterns"""
    a = np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)
    b = np.ascontiguousarray(y_ref, dtype=np.float64).view(np.uint64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.flatnonzero(a != b)


def assert_same_bits(y, y_ref, what="", row_info=None):
    """y and y_ref hold the same float64 bit patterns, element for element.  On failure the message names `what`, how
    many rows differ, and the first differing row with both values and both hex patterns (plus row_info(row) if given)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    y_ref = np.ascontiguousarray(y_ref, dtype=np.float64)
    assert y.shape == y_ref.shape, f"{what}: shape {y.shape} != {y_ref.shape}"
    bad = differing_rows(y, y_ref)
    if bad.size == 0:
        return
    i = int(bad[0])
    extra = f" ({row_info(i)})" if row_info is not None else ""
    raise AssertionError(f"{what}: {bad.size} of {y.size} rows differ in their bits; first row {i}{extra}: "
                         f"{y[i]!r} (0x{int(y.view(np.uint64)[i]):016x}) != expected {y_ref[i]!r} "
                         f"(0x{int(y_ref.view(np.uint64)[i]):016x})")
