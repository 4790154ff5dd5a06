"""Host checks (no GPU) that the inputs of tests/test_gpu_serial_order.py can fail: another order of a row's products, a
-0.0 seed, or column-sorting a row with a descending pair gives other bits than the serial oracle on them.  A kernel that
added in any of those orders would therefore not pass the GPU module."""
import numpy as np
import pytest

import serial_order_inputs as si
from bits import assert_same_bits, differing_rows


def _y(oracle, IRP, JA, AS, x, perm=None):
    if perm is not None:
        JA, AS = JA[perm], AS[perm]
    return oracle.csr_serial(IRP, JA, AS, x)


def _share(rows, mask):
    return np.isin(np.flatnonzero(mask), rows).mean() if mask.any() else 1.0


@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("name", ["mixed", "narrow17", "widespan"])
def test_inputs_see_the_order(oracle, name, unit):
    inp = si.make(name)
    if unit:
        inp = si.unit(inp)
    IRP, JA, AS, x = inp.IRP, inp.JA, inp.AS, inp.x
    assert JA.size >= si.AUTO_MIN_NNZ and inp.M % 4 != 0
    y = _y(oracle, IRP, JA, AS, x)
    assert_same_bits(_y(oracle, IRP, JA, AS, x), y, "the oracle is deterministic")
    lens = inp.lens()
    many = lens >= 3                        # two products give the same bits in either order (addition commutes)
    rev = differing_rows(_y(oracle, IRP, JA, AS, x, si.reversed_rows(IRP)), y)
    by_size = differing_rows(_y(oracle, IRP, JA, AS, x, si.stable_rows_by(IRP, np.abs(AS * x[JA.astype(np.int64)]))), y)
    assert _share(rev, many) > 0.6, "reversed rows"
    assert _share(by_size, many) > 0.45, "rows sorted by |a x|"
    if not unit:                            # equal columns: only the stored order of the run tells the entries apart
        runs = inp.special["run"]
        assert np.isin(runs, differing_rows(_y(oracle, IRP, JA, AS, x, si.runs_reversed(IRP, JA)), y)).mean() > 0.6
        if "long-run" in inp.special:
            assert np.isin(inp.special["long-run"], differing_rows(_y(oracle, IRP, JA, AS, x, si.runs_reversed(IRP, JA)), y)).all()
        # the cancelling runs are exactly +0.0
        c = inp.special["cancel"]
        assert np.all(y[c].view(np.uint64) == 0)
    assert lens[inp.special["empty"]].max() == 0 and {0, inp.M - 1} <= set(inp.special["empty"].tolist())
    # rows whose products are all -0.0: the oracle's +0.0 start makes them +0.0; a row seeded with its first product
    # would be -0.0
    if not unit:                            # (-2.5 x is no zero there)
        neg = np.concatenate([inp.special["negzero"], inp.special["negzero-single"]])
        assert np.all(y[neg].view(np.uint64) == 0)
        prods = AS * x[JA.astype(np.int64)]
        in_neg = np.isin(si.row_of_entry(IRP), neg)
        assert np.all(np.signbit(prods[in_neg]) & (prods[in_neg] == 0))
        # x holds both signed zeros, the values both too
        assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
        assert (np.signbit(AS) & (AS == 0)).any() and (~np.signbit(AS) & (AS == 0)).any()


@pytest.mark.parametrize("where", ["last-row", "63/64", "127/128"])
def test_descending_pair_changes_the_bits_when_sorted(oracle, where):
    M, N, IRP, JA, AS, x, row = si.descending_pair(where)
    J = JA.astype(np.int64)
    r = si.row_of_entry(IRP)
    desc = np.flatnonzero((J[1:] < J[:-1]) & (r[1:] == r[:-1]))
    assert desc.size == 1 and r[desc[0]] == row
    y = _y(oracle, IRP, JA, AS, x)
    assert differing_rows(_y(oracle, IRP, JA, AS, x, si.stripes_order(IRP, JA)), y).tolist() == [row]


def test_shuffled_rows_tell_the_two_deterministic_orders_apart(oracle):
    M, N, IRP, JA, AS, x = si.shuffled()
    many = np.diff(IRP.astype(np.int64)) >= 3
    y = _y(oracle, IRP, JA, AS, x)
    ys = _y(oracle, IRP, JA, AS, x, si.stripes_order(IRP, JA))
    yt = _y(oracle, IRP, JA, AS, x, si.tiles_order(IRP, JA))
    assert _share(differing_rows(ys, y), many) > 0.5
    assert _share(differing_rows(yt, y), many) > 0.4
    assert _share(differing_rows(yt, ys), many) > 0.25


def test_assert_same_bits_tells_signed_zeros_apart():
    assert_same_bits(np.array([0.0, 1.0]), np.array([0.0, 1.0]))
    with pytest.raises(AssertionError, match=r"first row 1.*0x8000000000000000"):
        assert_same_bits(np.array([1.0, -0.0]), np.array([1.0, 0.0]), "signed zero")
