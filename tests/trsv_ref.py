"""The test side's reference for the triangular solve (hipSpTRSVCSR, include/spmvHip.h): the serial loop

    lower: for i = 0, 1, ..., M-1            upper: for i = M-1, M-2, ..., 0
        acc = +0.0
        for p in IRP[i] .. IRP[i+1]-1   (stored order)
            j = JA[p]
            if (lower ? j < i : j > i):  acc += AS[p] * x[j]
        x[i] = STORED ? (b[i] - acc) / AS[diagPos[i]] : (b[i] - acc)

in plain Python for small inputs (`trsv_loop`), and a level-vectorised numpy form for large ones (`trsv_levels`): the rows
of one level are independent, so numpy walks them together position by position in stored order, skipping the positions
outside the triangle (never adding +0.0 in their place: -0.0 + 0.0 is +0.0).  Both round every product and every add
separately, as IEEE double does with no FMA."""
import numpy as np


def diag_pos(M, IRP, JA):
    """(diagPos, first bad row or -1): the position of row i's diagonal entry where it holds exactly one"""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    on = np.flatnonzero(JA == rows)
    count = np.bincount(rows[on], minlength=M)
    pos = np.zeros(M, dtype=np.int64)
    pos[rows[on]] = on
    bad = np.flatnonzero(count != 1)
    return pos, (int(bad[0]) if bad.size else -1)


def trsv_loop(M, IRP, JA, AS, b, lower=True, unit=False):
    """the loop above, one row and one entry at a time"""
    irp, ja, a = [int(v) for v in IRP], [int(v) for v in JA], [float(v) for v in AS]
    x = [float(v) for v in b]
    order = range(M) if lower else range(M - 1, -1, -1)
    for i in order:
        acc, d, nd = 0.0, None, 0
        for p in range(irp[i], irp[i + 1]):
            j = ja[p]
            if (j < i) if lower else (j > i):
                acc += a[p] * x[j]
            if j == i:
                d, nd = a[p], nd + 1
        r = x[i] - acc
        if unit:
            x[i] = r
        else:
            assert nd == 1, f"row {i}: {nd} diagonal entries"
            x[i] = _div(r, d)
    return np.array(x, dtype=np.float64)


def _div(r, d):
    """IEEE double division (Python raises on / 0.0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(r) / np.float64(d))


def levels(M, IRP, JA, lower=True):
    """level of every row: 0 without a strict-triangle entry, else 1 + the largest level of the rows it reads"""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    strict = (JA < rows) if lower else ((JA > rows) & (JA < M))
    src, dst = JA[strict], rows[strict]                 # row dst reads row src
    cnt = np.bincount(dst, minlength=M)
    o = np.argsort(src, kind="stable")
    dep_ptr = np.zeros(M + 1, dtype=np.int64)
    dep_ptr[1:] = np.cumsum(np.bincount(src, minlength=M))
    dep = dst[o]
    lvl = np.full(M, -1, dtype=np.int64)
    front = np.flatnonzero(cnt == 0)
    cnt = cnt.copy()
    level = 0
    while front.size:
        lvl[front] = level
        lens = dep_ptr[front + 1] - dep_ptr[front]
        idx = np.repeat(dep_ptr[front] - np.cumsum(lens) + lens, lens) + np.arange(lens.sum())
        q = dep[idx]
        np.subtract.at(cnt, q, 1)
        q = np.unique(q)
        front = q[cnt[q] == 0]
        level += 1
    assert (lvl >= 0).all()
    return lvl


def trsv_levels(M, IRP, JA, AS, b, lower=True, unit=False, lvl=None):
    """the loop above, vectorised over the rows of each level (same bits)"""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    AS = np.asarray(AS, dtype=np.float64)
    x = np.array(b, dtype=np.float64, copy=True)
    if M == 0:
        return x
    if lvl is None:
        lvl = levels(M, IRP, JA, lower)
    if not unit:
        dpos, bad = diag_pos(M, IRP, JA)
        assert bad < 0, f"row {bad} does not hold exactly one diagonal entry"
    order = np.argsort(lvl, kind="stable")
    bounds = np.searchsorted(lvl[order], np.arange(lvl.max() + 2))
    with np.errstate(all="ignore"):
        for l in range(lvl.max() + 1):
            R = order[bounds[l]:bounds[l + 1]]
            s, lens = IRP[R], IRP[R + 1] - IRP[R]
            acc = np.zeros(R.size)
            for k in range(int(lens.max()) if R.size else 0):
                live = np.flatnonzero(k < lens)
                p = s[live] + k
                j = JA[p]
                tri = (j < R[live]) if lower else ((j > R[live]) & (j < M))
                live, p, j = live[tri], p[tri], j[tri]
                acc[live] = acc[live] + AS[p] * x[j]
            r = x[R] - acc
            x[R] = r if unit else r / AS[dpos[R]]
    return x
