"""The exact reference (tests/exact_ref.py) on the host: exact_rows is the correctly rounded exact row sum (checked with
fractions.Fraction), the serial oracle meets check_any_order on every family and value kind of the sequence test, and
check_any_order rejects every subtly wrong result the sequence test must be able to tell from a right one."""
from fractions import Fraction

import numpy as np
import pytest

import exact_ref
from exact_ref import check_any_order, exact_rows
from sequence_inputs import FAMILIES, KINDS, family, values


def _fraction_rows(IRP, JA, AS, x):
    out = []
    for i in range(IRP.size - 1):
        s = Fraction(0)
        for p in range(int(IRP[i]), int(IRP[i + 1])):
            s += Fraction(float(AS[p])) * Fraction(float(x[int(JA[p])]))
        out.append(float(s))                    # Fraction -> float rounds once, to nearest even
    return np.array(out) + 0.0


def _small(rng, case):
    M, N = 40, 12
    lens = rng.integers(0, 9, M)
    lens[[0, 5]] = 0
    IRP = np.zeros(M + 1, dtype=np.uint64)
    IRP[1:] = np.cumsum(lens)
    nnz = int(IRP[-1])
    JA = rng.integers(0, N, nnz).astype(np.uint64)       # unsorted, repeated columns
    x = rng.uniform(-1, 1, N) * 2.0 ** rng.integers(-30, 31, N)
    if case == "random":
        AS = rng.uniform(-1, 1, nnz)
    elif case == "spread":                               # magnitudes over 2^+-150
        AS = rng.choice([-1.0, 1.0], nnz) * 2.0 ** rng.uniform(-150, 150, nnz)
        x = rng.choice([-1.0, 1.0], N) * 2.0 ** rng.uniform(-40, 40, N)
    elif case == "cancel":                               # +v / -v on the same column: rows that cancel to exactly zero
        half = rng.uniform(-1, 1, nnz)
        AS = half.copy()
        for i in range(M):
            s, t = int(IRP[i]), int(IRP[i + 1])
            for p in range(s + 1, t, 2):
                JA[p] = JA[p - 1]
                AS[p] = -AS[p - 1]
    elif case == "huge":                                 # one huge term among tiny ones
        AS = rng.uniform(-1, 1, nnz) * 2.0 ** -120
        AS[rng.integers(nnz, size=M // 4)] = 2.0 ** 110
    else:
        raise KeyError(case)
    return IRP, JA, AS, x


@pytest.mark.parametrize("case", ["random", "spread", "cancel", "huge"])
@pytest.mark.parametrize("seed", range(4))
def test_exact_rows_is_the_rounded_exact_sum(case, seed):
    IRP, JA, AS, x = _small(np.random.default_rng(seed * 10 + len(case)), case)
    got = exact_rows(IRP, JA, AS, x)
    want = _fraction_rows(IRP, JA, AS, x)
    assert got.tobytes() == want.tobytes()
    if case == "cancel":
        assert (got[np.diff(IRP.astype(np.int64)) % 2 == 0] == 0).all()
    assert np.signbit(got[[0, 5]]).sum() == 0             # empty rows: +0.0


def test_two_products_are_exact():
    rng = np.random.default_rng(3)
    a = rng.choice([-1.0, 1.0], 2000) * 2.0 ** rng.uniform(-200, 200, 2000)
    b = rng.choice([-1.0, 1.0], 2000) * 2.0 ** rng.uniform(-200, 200, 2000)
    p, e = exact_ref.two_products(a, b)
    for k in range(a.size):
        assert Fraction(float(p[k])) + Fraction(float(e[k])) == Fraction(float(a[k])) * Fraction(float(b[k]))


def test_out_of_range_is_refused():
    IRP = np.array([0, 2], dtype=np.uint64)
    JA = np.array([0, 1], dtype=np.uint64)
    with pytest.raises(AssertionError, match="outside"):
        exact_rows(IRP, JA, np.array([1.0, 2.0 ** -210]), np.ones(2))
    with pytest.raises(AssertionError, match="outside"):
        exact_rows(IRP, JA, np.ones(2), np.array([2.0 ** 201, 1.0]))
    with pytest.raises(AssertionError, match="NaN or Inf"):
        exact_rows(IRP, JA, np.ones(2), np.array([np.inf, 1.0]))


def test_bound_is_gamma_n_plus_one():
    """one row of n products: the bound allows gamma(n + 1) * sum|a x| and not a bit more"""
    IRP = np.array([0, 3], dtype=np.uint64)
    JA = np.array([0, 1, 2], dtype=np.uint64)
    AS = np.array([1.0, 1.0, 1.0])
    x = np.array([1.0, 2.0 ** -60, 2.0 ** -60])
    check_any_order(IRP, JA, AS, x, np.array([1.0]), "rounded sum")
    allowed = exact_ref.gamma(4) * 1.0
    check_any_order(IRP, JA, AS, x, np.array([1.0 + 2.0 ** -52]), "one ulp up: within 4u")
    assert 2.0 ** -52 - 2.0 ** -59 <= allowed
    with pytest.raises(AssertionError, match="row 0 \\(n_i = 3\\)"):
        check_any_order(IRP, JA, AS, x, np.array([1.0 + 2.0 ** -50]), "four ulps up")
    with pytest.raises(AssertionError, match="non-finite"):
        check_any_order(IRP, JA, AS, x, np.array([np.nan]), "nan")


def test_zero_rows_must_be_zero():
    IRP = np.array([0, 0, 2], dtype=np.uint64)
    JA = np.array([0, 1], dtype=np.uint64)
    AS = np.array([0.0, -0.0])
    x = np.array([1.0, 3.0])
    check_any_order(IRP, JA, AS, x, np.array([0.0, -0.0]), "zeros")
    with pytest.raises(AssertionError, match="row 1"):
        check_any_order(IRP, JA, AS, x, np.array([0.0, 2.0 ** -1000]), "zero row off by a hair")


# ---------------------------------------------------------------- the families of the sequence test
def _case(fam, kind, seed=0):
    M, N, IRP, JA, x0, x1 = family(fam)
    rng = np.random.default_rng(1000 * FAMILIES.index(fam) + 10 * KINDS.index(kind) + seed)
    return M, N, IRP, JA, values(rng, kind, IRP, JA, x0), x0, x1, rng


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_serial_oracle_meets_the_bound(oracle, fam, kind):
    """sgemvSerial (one order of the sums) passes check_any_order on every family, value kind and x of the GPU test"""
    M, N, IRP, JA, AS, x0, x1, _ = _case(fam, kind)
    for x in (x0, x1):
        check_any_order(IRP, JA, AS, x, oracle.csr_serial(IRP, JA, AS, x), f"{fam}/{kind}")


def _rows_caught(IRP, JA, AS, x, y, rows):
    """how many of `rows` check_any_order rejects, row by row (one row checked at a time, the others made right)"""
    caught = 0
    for i in rows:
        s, t = int(IRP[i]), int(IRP[i + 1])
        sub = np.array([0, t - s], dtype=np.uint64)
        try:
            check_any_order(sub, JA[s:t], AS[s:t], x, y[i:i + 1], "row")
        except AssertionError:
            caught += 1
    return caught


def _mutant(oracle, mutation, IRP, JA, AS, x, rng, N, old):
    """(y of the made-up wrong kernel, the rows it changed)"""
    lens = np.diff(IRP.astype(np.int64))
    rows = rng.choice(np.flatnonzero(lens >= 2), 64, replace=False)
    y = oracle.csr_serial(IRP, JA, AS, x)
    if mutation == "value_before_update":
        return oracle.csr_serial(IRP, JA, old, x), rows
    if mutation == "unit_value_of_a_non_unit_handle":
        return oracle.csr_serial(IRP, JA, np.full(AS.size, AS[0]), x), rows
    for i in rows:
        s, t = int(IRP[i]), int(IRP[i + 1])
        p = int(rng.integers(s, t))
        a, j = AS[s:t].copy(), JA[s:t].copy()
        if mutation == "dropped_product":
            a[p - s] = 0.0
        elif mutation == "doubled_product":
            a = np.append(a, AS[p])
            j = np.append(j, JA[p])
        elif mutation == "read_x_j_plus_1":
            j[p - s] = (int(JA[p]) + 1) % N
        else:
            raise KeyError(mutation)
        y[i] = oracle.csr_serial(np.array([0, a.size], dtype=np.uint64), j, a, x)[0]
    return y, rows


MUTATIONS = ("dropped_product", "doubled_product", "read_x_j_plus_1", "value_before_update", "unit_value_of_a_non_unit_handle")


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_check_any_order_rejects_a_wrong_kernel(oracle, fam, mutation):
    """Each made-up wrong result is refused by check_any_order on every value kind it applies to, caught on at least one
    changed row (and on most of them: the report says how many)."""
    for k, kind in enumerate(KINDS):
        M, N, IRP, JA, AS, x0, x1, rng = _case(fam, kind, 1)
        if kind.startswith("constant") and mutation == "unit_value_of_a_non_unit_handle":
            continue                                     # (the unit value IS right for a near-unit matrix's most rows)
        old = values(rng, KINDS[(k + 1) % len(KINDS)], IRP, JA, x0)
        x = (x0, x1)[k % 2]
        y, rows = _mutant(oracle, mutation, IRP, JA, AS, x, rng, N, old)
        if kind == "constant" and AS[0] == 0.0 and mutation != "value_before_update":
            continue                                     # (all products zero: no wrong product to see)
        with pytest.raises(AssertionError, match=f"{fam}/{kind}"):
            check_any_order(IRP, JA, AS, x, y, f"{fam}/{kind}")
        assert _rows_caught(IRP, JA, AS, x, y, rows) >= 1, (fam, kind, mutation)
