"""NumPy restatement of the portfolio loss (include/tcrisk_hip.h, "portfolio loss" section), written from the model statement
alone: the Emanuel (2011) damage function on a matrix of footprint peak winds, its sums, and the loss curves."""
import math

import numpy as np

U = 2.0 ** -52


def damage(m, v_thresh, v_half):
    """D = x^3 / (1 + x^3), x = max(m - v_thresh, 0) / (v_half - v_thresh); 0 where m is NaN."""
    m = np.asarray(m, float)
    with np.errstate(invalid='ignore'):
        x = np.where(np.isnan(m), 0.0, np.maximum(m - v_thresh, 0.0)) / (np.asarray(v_half, float) - v_thresh)
    x3 = x * x * x
    return x3 / (1.0 + x3)


def loss_matrix(site_max, value, v_thresh, v_half):
    """T[i][s] = value[i] D(site_max[i][s]); v_half a scalar or one per site."""
    vh = np.asarray(v_half, float)
    vh = vh[:, None] if vh.ndim else vh
    return np.asarray(value, float)[:, None] * damage(site_max, v_thresh, vh)


def exact_sums(T, axis):
    """The exactly rounded sums of T along an axis (math.fsum)."""
    T = np.asarray(T, float)
    rows = T.T if axis == 0 else T
    return np.array([math.fsum(r) for r in rows])


def year_table(event_loss, groups, n_groups):
    """(agg, max, n) per group: exactly rounded sum, maximum (0 without storms) and number of storms."""
    e, g = np.asarray(event_loss, float), np.asarray(groups)
    agg = np.array([math.fsum(e[g == k]) for k in range(n_groups)])
    mx = np.array([e[g == k].max() if (g == k).any() else 0.0 for k in range(n_groups)])
    return agg, mx, np.array([(g == k).sum() for k in range(n_groups)])


def loss_curve(year_losses, total_years, return_periods):
    """The k-th largest of the year losses padded with zero years to total_years, k the smallest integer with k T >= total_years;
    NaN for T > total_years."""
    y = sorted(list(np.asarray(year_losses, float)) + [0.0] * (total_years - len(year_losses)), reverse=True)
    out = []
    for T in return_periods:
        if T > total_years:
            out.append(np.nan)
            continue
        k = 1
        while k * T < total_years:
            k += 1
        out.append(y[min(k, total_years) - 1])                  # T < 1: every year, the smallest year loss
    return np.array(out)
