"""numpy restatement of an f16x3 statistics block (cnslmat/f16-split.h:
ebits, spread, small_bound; kaldi-lite/cu-f16-stats.hip: the comment at
its head; kaldi-lite/f16-stats.h: struct StatOp).

A scale group is a row or a column of a float32 matrix.  Its block entry is
[max, min, cnt], three uint32 words:

  max  the largest |x| bit pattern of the group (Inf / NaN: >= 0x7f800000);
  min  the smallest nonzero |x| bit pattern, 0 when the group has none;
  cnt  for a spread group the number of its nonzero elements with
       |x| < 2^(ebits(max) - 17) (small_bound: 2^-3 after the group's scale,
       which puts max in [2^14, 2^15)); 0 for every other group.

A group is spread when min != 0, max is finite and ebits(min) <
ebits(max) - 20; ebits is the exponent of a nonzero |x| bit pattern, a
subnormal's taken from its leading bit.  Everything here is integer
arithmetic on the bit patterns: the bound 2^k compares as ebits(x) < k."""
import numpy as np

NONFINITE = 0x7F800000


def ebits(b):
    """f16-split.h ebits over an array of nonzero |x| bit patterns."""
    b = np.asarray(b).astype(np.int64)
    # frexp of an integer below 2^53 is exact: b = m 2^e with m in [0.5, 1),
    # so the leading bit of b is bit e - 1
    lead = np.frexp(np.maximum(b, 1).astype(np.float64))[1].astype(np.int64) - 1
    return np.where(b >= 0x00800000, (b >> 23) - 127, lead - 149)


def abs_bits(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)


def spread(mx, mn):
    """f16-split.h spread over arrays of max / min bit patterns."""
    mx, mn = np.asarray(mx).astype(np.int64), np.asarray(mn).astype(np.int64)
    return (mn != 0) & (mx < NONFINITE) & (ebits(np.maximum(mn, 1)) < ebits(np.maximum(mx, 1)) - 20)


def stats_parts(x, axis):
    """(max, min, cnt) as uint32 arrays, one entry per row (axis 1: the
    reduction runs along the row) or per column (axis 0) of a 2-D float32
    array."""
    a = abs_bits(x)
    assert a.ndim == 2 and axis in (0, 1)
    if axis == 0:
        a = a.T
    n = a.shape[0]
    if a.shape[1] == 0:
        z = np.zeros(n, np.uint32)
        return z, z.copy(), z.copy()
    mx = a.max(1)
    big = np.int64(1) << 32
    mn = np.where(a == 0, big, a).min(1)
    mn = np.where(mn == big, 0, mn)
    spr = spread(mx, mn)
    e = ebits(np.maximum(mx, 1))
    # |x| < 2^(e - 17), x nonzero: a power-of-two bound is a bound on ebits
    small = (a != 0) & (ebits(np.maximum(a, 1)) < (e - 17)[:, None])
    cnt = np.where(spr, small.sum(1), 0)
    return mx.astype(np.uint32), mn.astype(np.uint32), cnt.astype(np.uint32)


def stats_block(x, axis):
    """The statistics block [max[n], min[n], cnt[n]] (3 n uint32 words) of the
    rows (axis=1) or the columns (axis=0) of x."""
    return np.concatenate(stats_parts(x, axis))
