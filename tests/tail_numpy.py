"""NumPy restatement of the row tail fit (include/tcrisk_hip.h, "row tail fit (return levels past the record)"): per row, a
generalized Pareto distribution fitted by probability-weighted moments to the excesses of the k largest values over the (k+1)-th,
and the levels of the return periods read off the fit.  Written from the header's text, step by step and in its order: every
operation of steps 1 to 5 is one IEEE fp64 operation on Python floats or NumPy scalars (no np.sum, no fused operation), so the
threshold, xi and sigma are compared bit for bit; step 6 goes through log and expm1 and gets a tolerance."""
import math

import numpy as np

from tests import levels_numpy as LN


def tree_sum(v):
    """The header's fixed tree: pad with +0.0 to the next power of two >= len(v) (at least 2), then s[i] = s[2i] + s[2i+1] until one
    value is left."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    P = 2
    while P < v.size:
        P *= 2
    s = np.zeros(P)
    s[:v.size] = v
    with np.errstate(invalid='ignore', over='ignore'):
        while s.size > 1:
            s = s[0::2] + s[1::2]                     # elementwise: one IEEE addition per pair
    return float(s[0])


def excesses(row, k):
    """(n_valid, u, y [k] ascending) of one row; u NaN and y None when the row holds fewer than k + 1 values that are not NaN."""
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    key = np.sort(LN.keys(row[~np.isnan(row)]))[::-1]                       # descending, in the key order
    if key.size < k + 1:
        return key.size, np.nan, None
    u = LN.values(key[k:k + 1])[0]
    x = LN.values(key[:k][::-1])                                            # the k largest (ties at u included), ascending
    with np.errstate(invalid='ignore'):
        return key.size, u, x - u


def pwm(y):
    """(xi, sigma) of ascending excesses by steps 4 and 5; (NaN, NaN) when the fit is undefined."""
    k = y.size
    w = np.array([float(k - i) for i in range(1, k + 1)])
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        S0 = tree_sum(y)
        S1 = tree_sum(w * y)
        a0 = np.float64(S0) / np.float64(k)
        a1 = np.float64(S1) / (np.float64(k) * np.float64(k - 1))
        d = a0 - np.float64(2.0) * a1
        if not (d > 0 and a1 > 0):
            return np.nan, np.nan
        xi = np.float64(2.0) - a0 / d
        sigma = ((np.float64(2.0) * a0) * a1) / d
    return float(xi), float(sigma)


def log_periods(k, total_years, periods):
    """L_j of step 6."""
    return np.array([math.log((float(k) / float(total_years)) * float(T)) for T in np.asarray(periods, dtype=np.float64).reshape(-1)])


def row_tail(plane, k, total_years, periods):
    """dict(threshold, xi, sigma [n_row], level [n_row][n_T], n_valid [n_row] int32) of levels.row_tail."""
    plane = np.asarray(plane, dtype=np.float64)
    L = log_periods(k, total_years, periods)
    n_row = plane.shape[0]
    out = dict(threshold=np.full(n_row, np.nan), xi=np.full(n_row, np.nan), sigma=np.full(n_row, np.nan),
               level=np.full((n_row, L.size), np.nan), n_valid=np.zeros(n_row, np.int32))
    for r, row in enumerate(plane):
        out['n_valid'][r], u, y = excesses(row, k)
        out['threshold'][r] = u
        if y is None:
            continue
        xi, sigma = pwm(y)
        out['xi'][r], out['sigma'][r] = xi, sigma
        if math.isnan(xi):
            continue
        for j, Lj in enumerate(L):
            if Lj < 0:
                continue
            out['level'][r, j] = u + sigma * Lj if xi == 0 else u + sigma * math.expm1(xi * Lj) / xi
    return out
