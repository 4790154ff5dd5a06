"""The test side's stable transpose of a CSR matrix (what spmvHipCsrTranspose promises), and the textbook scatter loop
whose bits hipSpMVRowsCSR on the transpose must give.

Row j of A^T holds the entries of column j of A in their CSR position order: ascending source row, and within a row the
stored order (unsorted rows and repeated (i, j) pairs included) -- a stable argsort of JA."""
import numpy as np

from serial_order_inputs import row_of_entry


def stable_transpose(N, IRP, JA, AS):
    """(IRPt u64, JAt u64 = source rows, ASt f64, order) of the N-row transpose; ASt = AS[order]"""
    JA = np.asarray(JA).astype(np.int64)
    order = np.argsort(JA, kind="stable")
    IRPt = np.zeros(N + 1, dtype=np.uint64)
    IRPt[1:] = np.cumsum(np.bincount(JA, minlength=N))
    rows = row_of_entry(np.asarray(IRP))
    return IRPt, rows[order].astype(np.uint64), np.asarray(AS, dtype=np.float64)[order], order


def scatter_serial(M, N, IRP, JA, AS, x):
    """y = +0.0;  for i in 0..M-1: for p in IRP[i]..IRP[i+1]-1: y[JA[p]] += AS[p] * x[i]   (IEEE double, in that order)"""
    y = [0.0] * N
    irp, ja, a, xs = [int(v) for v in IRP], [int(v) for v in JA], list(map(float, AS)), list(map(float, x))
    for i in range(M):
        for p in range(irp[i], irp[i + 1]):
            y[ja[p]] += a[p] * xs[i]
    return np.array(y, dtype=np.float64)
