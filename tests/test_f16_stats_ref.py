"""f16_stats_ref.stats_block (the numpy definition of an f16x3 statistics
block the GPU tests compare the kernels with) against hand-written groups:
every expected word below is worked out from f16-split.h's definitions by
hand, not by the module."""
import numpy as np

from f16_stats_ref import ebits, stats_block, stats_parts

F = np.float32
INF = 0x7F800000


def bits(v):
    return int(np.array([abs(F(v))], np.float32).view(np.uint32)[0])


def from_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def one(group):
    """(max, min, cnt) of one group, the same as a row and as a column."""
    g = np.asarray(group, np.float32)
    r = [int(p[0]) for p in stats_parts(g[None, :], 1)]
    c = [int(p[0]) for p in stats_parts(g[:, None], 0)]
    assert r == c, (r, c)
    return tuple(r)


def test_ebits():
    b = np.array([1, 2, 3, 0x400000, 0x7FFFFF, 0x800000, 0x3F800000, 0x7F7FFFFF])
    assert ebits(b).tolist() == [-149, -148, -148, -127, -127, -126, 0, 127]


def test_all_zero():
    assert one([0.0, 0.0, 0.0]) == (0, 0, 0)


def test_one_element():
    assert one([1.5]) == (0x3FC00000, 0x3FC00000, 0)
    assert one([0.0]) == (0, 0, 0)
    assert one([-2.0]) == (0x40000000, 0x40000000, 0)


def test_negative_zero():
    # -0.0 is a zero: neither the max's sign bit nor a nonzero minimum
    assert one([-0.0, 0.0]) == (0, 0, 0)
    assert one([-0.0, -3.0, 0.5]) == (0x40400000, 0x3F000000, 0)


def test_nan_and_inf():
    mx, mn, cnt = one([1.0, np.nan, 2.0 ** -40])
    assert mx >= INF and mx == 0x7FC00000 and mn == bits(2.0 ** -40) and cnt == 0
    for v in (np.inf, -np.inf):
        mx, mn, cnt = one([1.0, v, 2.0 ** -40, 2.0 ** -41])
        assert mx == INF and mn == bits(2.0 ** -41) and cnt == 0


def test_subnormal_max():
    # max 2^-140 (bit 9 of the fraction): exponent -140 by its leading bit;
    # nothing can lie 21 binades below it, so never spread
    assert one([from_bits(0x200), from_bits(1), 0.0]) == (0x200, 1, 0)
    # max 2^-127 (subnormal), min 2^-149: 22 binades, spread; the bound is
    # 2^-144: 2^-149 and 2^-145 are counted, 2^-144 is not
    g = [from_bits(0x400000), from_bits(1), from_bits(0x10), from_bits(0x20)]
    assert one(g) == (0x400000, 1, 2)


def test_twenty_binades():
    # min exactly 20 binades below the max (any fraction bits): not spread
    assert one([1.75, 2.0 ** -20]) == (bits(1.75), bits(2.0 ** -20), 0)
    assert one([1.0, 1.5 * 2.0 ** -20, -(2.0 ** -18)]) == (0x3F800000, bits(1.5 * 2.0 ** -20), 0)
    # exactly 21 below: spread; bound 2^-17: 2^-21 and 2^-18 count
    assert one([1.75, 1.99 * 2.0 ** -21]) == (bits(1.75), bits(1.99 * 2.0 ** -21), 1)
    assert one([1.0, 2.0 ** -21, -(2.0 ** -18), 0.0]) == (0x3F800000, bits(2.0 ** -21), 2)


def test_small_bound_edge():
    # max in [2^3, 2^4): e = 3, bound 2^-14
    at = F(2.0 ** -14)
    below = from_bits(bits(at) - 1)
    tiny = F(2.0 ** -30)
    assert one([8.0, tiny, at]) == (bits(8.0), bits(tiny), 1)       # at the bound: not counted
    assert one([15.5, tiny, below]) == (bits(15.5), bits(tiny), 2)  # one ulp below: counted
    assert one([-8.0, -tiny, -below, at, 0.0, -0.0]) == (bits(8.0), bits(tiny), 2)


def test_block_layout():
    x = np.array([[1.0, 0.0, -4.0],
                  [2.0 ** -30, 0.0, 0.5]], np.float32)
    rows = stats_block(x, 1)
    assert rows.dtype == np.uint32
    assert rows.tolist() == [bits(4.0), bits(0.5), bits(1.0), bits(2.0 ** -30), 0, 1]
    cols = stats_block(x, 0)
    assert cols.tolist() == [bits(1.0), 0, bits(4.0), bits(2.0 ** -30), 0, bits(0.5), 1, 0, 0]
    assert stats_block(np.zeros((0, 3), np.float32), 0).tolist() == [0] * 9
    assert stats_block(np.zeros((2, 0), np.float32), 1).tolist() == [0] * 6
