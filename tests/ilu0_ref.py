"""The test side's reference for the ILU(0) factorisation (hipSpILU0CSR, include/spmvHip.h): the serial loop

    for i = 0, 1, ..., M-1
        for p = IRP[i] .. diagPos[i]-1                 -- k = JA[p] < i, ascending
            k = JA[p]
            AS[p] = AS[p] / AS[diagPos[k]]             -- row k is final
            for q = p+1 .. IRP[i+1]-1                   -- j = JA[q] > k, ascending
                if row k stores column JA[q] at position r:
                    AS[q] = AS[q] - AS[p] * AS[r]

in plain Python for small inputs (`ilu0_loop`), and a level-vectorised numpy form for large ones (`ilu0_levels`): the rows
of one lower level read only rows of earlier levels, so numpy walks them together through their k positions, rounding
every product and every subtraction separately, as IEEE double does with no FMA.  Both need every row's columns strictly
ascending and exactly one diagonal entry per row (the library refuses anything else)."""
import numpy as np

from trsv_ref import _div, diag_pos, levels


def check_pattern(M, IRP, JA):
    """(diagPos, first row that is not strictly ascending or -1, first row without exactly one diagonal or -1)"""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    step = np.flatnonzero((rows[1:] == rows[:-1]) & (JA[1:] <= JA[:-1]))
    dpos, bad_diag = diag_pos(M, IRP, JA)
    return dpos, (int(rows[step[0]]) if step.size else -1), bad_diag


def ilu0_loop(M, IRP, JA, AS):
    """the loop above, one row, one k and one entry at a time"""
    dpos, unsorted, bad = check_pattern(M, IRP, JA)
    assert unsorted < 0 and bad < 0, (unsorted, bad)
    irp, ja, a = [int(v) for v in IRP], [int(v) for v in JA], [float(v) for v in AS]
    where = [{ja[r]: r for r in range(irp[k], irp[k + 1])} for k in range(M)]
    d = [int(v) for v in dpos]
    for i in range(M):
        for p in range(irp[i], d[i]):
            k = ja[p]
            a[p] = _div(a[p], a[d[k]])
            wk = where[k]
            for q in range(p + 1, irp[i + 1]):
                r = wk.get(ja[q])
                if r is not None:
                    a[q] = a[q] - a[p] * a[r]
    return np.array(a, dtype=np.float64)


def ilu0_levels(M, IRP, JA, AS, lvl=None):
    """the loop above, vectorised over the rows of each lower level (same bits)"""
    IRP = np.asarray(IRP, dtype=np.int64)
    JA = np.asarray(JA, dtype=np.int64)
    a = np.array(AS, dtype=np.float64, copy=True)
    if M == 0:
        return a
    dpos, unsorted, bad = check_pattern(M, IRP, JA)
    assert unsorted < 0 and bad < 0, (unsorted, bad)
    if lvl is None:
        lvl = levels(M, IRP, JA, True)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    keys = rows * M + JA                                  # ascending: rows in order, columns strictly ascending
    order = np.argsort(lvl, kind="stable")
    bounds = np.searchsorted(lvl[order], np.arange(lvl.max() + 2))
    with np.errstate(all="ignore"):
        for l in range(lvl.max() + 1):
            R = order[bounds[l]:bounds[l + 1]]
            s, e, nlow = IRP[R], IRP[R + 1], dpos[R] - IRP[R]
            for t in range(int(nlow.max()) if R.size else 0):
                live = np.flatnonzero(t < nlow)
                p, end = s[live] + t, e[live]
                k = JA[p]
                a[p] = a[p] / a[dpos[k]]
                cnt = end - p - 1                         # q = p+1 .. end-1 of each live row
                own = np.repeat(np.arange(live.size), cnt)
                q = np.repeat(p + 1 - np.cumsum(cnt) + cnt, cnt) + np.arange(cnt.sum())
                want = k[own] * M + JA[q]
                r = np.minimum(np.searchsorted(keys, want), keys.size - 1)
                hit = keys[r] == want
                q, r, own = q[hit], r[hit], own[hit]
                a[q] = a[q] - a[p[own]] * a[r]
    return a


def ilu0_crout(M, IRP, JA, AS):
    """NOT the contract: the same factors with each entry's updates summed first and subtracted once (the 'dot-product'
    form, acc += AS[p] * AS[r] then AS[q] - acc).  Exact arithmetic agrees; rounding does not."""
    dpos, _, _ = check_pattern(M, IRP, JA)
    irp, ja, a = [int(v) for v in IRP], [int(v) for v in JA], [float(v) for v in AS]
    where = [{ja[r]: r for r in range(irp[k], irp[k + 1])} for k in range(M)]
    d = [int(v) for v in dpos]
    for i in range(M):
        acc = {}
        for p in range(irp[i], irp[i + 1]):
            j = ja[p]
            v = a[p] - acc[p] if p in acc else a[p]
            if j < i:
                v = _div(v, a[d[j]])
                for q in range(p + 1, irp[i + 1]):
                    r = where[j].get(ja[q])
                    if r is not None:
                        acc[q] = acc.get(q, 0.0) + v * a[r]
            a[p] = v
    return np.array(a, dtype=np.float64)


def ilu0_kij(M, IRP, JA, AS):
    """the right-looking (KIJ) order: for each k, every later row i that stores (i, k) is divided and updated.  It applies
    each entry's updates in the same ascending-k order as the loop, so it gives the same bits (see test_ilu0_abi)."""
    dpos, _, _ = check_pattern(M, IRP, JA)
    irp, ja, a = [int(v) for v in IRP], [int(v) for v in JA], [float(v) for v in AS]
    where = [{ja[r]: r for r in range(irp[i], irp[i + 1])} for i in range(M)]
    d = [int(v) for v in dpos]
    for k in range(M):
        for i in range(k + 1, M):
            p = where[i].get(k)
            if p is None:
                continue
            a[p] = _div(a[p], a[d[k]])
            for r in range(d[k] + 1, irp[k + 1]):
                q = where[i].get(ja[r])
                if q is not None:
                    a[q] = a[q] - a[p] * a[r]
    return np.array(a, dtype=np.float64)
