"""NumPy restatement of row selection (include/tcrisk_hip.h, "row selection (return levels)"): the k-th largest value of every
row that is not NaN, in the order of the order-preserving key of a double.  Written from the header's text: map to keys, sort the
keys with np.sort, index, map back.  No value is touched by arithmetic, so everything is compared bit for bit."""
import numpy as np

SIGN = np.uint64(1) << np.uint64(63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys(values):
    """uint64 keys of fp64 values: every bit flipped for a negative (sign bit set), the sign bit flipped otherwise."""
    b = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b & SIGN != 0, ALL, SIGN)


def values(k):
    """The inverse of keys."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return (k ^ np.where(k & SIGN != 0, SIGN, ALL)).view(np.float64)


def row_select(plane, ranks):
    """(level [n_row][n_rank], n_valid [n_row] int32): level[r][j] the ranks[j]-th largest non-NaN value of row r, NaN when the
    row holds fewer."""
    plane = np.asarray(plane, dtype=np.float64)
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    level = np.full((plane.shape[0], ranks.size), np.nan)
    n_valid = np.zeros(plane.shape[0], np.int32)
    for r, row in enumerate(plane):
        k = np.sort(keys(row[~np.isnan(row)]))[::-1]                 # descending
        n_valid[r] = k.size
        have = ranks <= k.size
        level[r, have] = values(k[ranks[have] - 1])
    return level, n_valid


def same_bits(a, b):
    """Elementwise: the same bits, or both NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.shape == b.shape) and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
