"""NumPy restatement of the rain-accumulation-window contract (include/tcrisk_hip.h "rain accumulation windows",
tropical_cyclone_risk_amd/accumulation.py), the definition written directly on the rainfall restatement (tests/rainfall_numpy.py:
its records, its rate, its distance, its r_out band and its tolerance).

For a site and a storm of n samples and nr = (n - 1) substeps + 1 records: rho_q is the rate of record q if it is within r_out,
else an exact 0.0; I_q = (h / 2)(rho_q + rho_q+1) with h = dt_s / (3600 substeps); T_k = I_0 + ... + I_(k substeps - 1), summed
sequentially in ascending q (np.cumsum, not np.sum's pairwise order), T_0 = 0; A(m) = max over k of T_k - T_max(k - m, 0).  NaN
when no record is within r_out.

A pair whose distance is within BAND_KM of r_out is ambiguous: `site_windows` counts those pairs, and the tests choose inputs
that have none.

Tolerance.  rainfall_numpy's TOL_ABS + TOL_REL |value|, and its argument: every term I_q is >= 0 and has a relative error of a
few ulp; T_k is a sequential sum of at most ~150 of them at the test shapes (48 samples x 3 sub-steps; 361 golden samples x 1),
so its error is about 1e-13 T_k; A is one subtraction of two such sums, whose errors are both relative to T_k <= the storm
total, not to A.  Where A is a small difference of large T the bound to use is TOL_ABS + TOL_REL total (`close_to`).
"""
import numpy as np

from tests import rainfall_numpy as RN
from tests.rainfall_numpy import BAND_KM, TOL_ABS, TOL_REL  # noqa: F401


def half_step(dt_s, substeps):
    """h / 2 in hours."""
    return (dt_s / (3600.0 * substeps)) / 2


def series(rec, site_lon, site_lat, r_out_km, dt_s, substeps, **prof):
    """Of one storm's records (RN.records(...)[s]) at the sites: (inside [n_site][nr] bool, rho [n_site][nr], I [n_site][nr - 1],
    T [n_site][n], the distances [n_site][nr])."""
    site_lon, site_lat = np.asarray(site_lon, float).reshape(-1), np.asarray(site_lat, float).reshape(-1)
    lo, la, vv, _ = (x[None, :] for x in rec)
    r = RN.haversine_km(lo, la, site_lon[:, None], site_lat[:, None])
    inside = r <= r_out_km
    rho = np.where(inside, RN.rate(r, vv, **prof), 0.0)
    I = half_step(dt_s, substeps) * (rho[:, :-1] + rho[:, 1:])
    S = np.concatenate([np.zeros((site_lon.size, 1)), np.cumsum(I, axis=1)], axis=1)         # sequential, in record order
    return inside, rho, I, S[:, ::substeps], r


def window_max(T, m):
    """[n_site]: max over k of T_k - T_max(k - m, 0), T [n_site][n]."""
    k = np.arange(T.shape[1])
    return (T - T[:, np.maximum(k - int(m), 0)]).max(axis=1)


def site_windows(recs, site_lon, site_lat, r_out_km, dt_s, substeps, window_samples, **prof):
    """(A [n_window][n_site][n_trk] in mm, NaN where the storm has no record within r_out_km of the site; n_band: the number of
    (site, record) pairs within BAND_KM of r_out_km)."""
    site_lon = np.asarray(site_lon, float).reshape(-1)
    A = np.full((len(window_samples), site_lon.size, len(recs)), np.nan)
    n_band = 0
    for s, rec in enumerate(recs):
        if rec is None:
            continue
        assert rec.shape[1] % substeps == 1 % substeps
        inside, _, _, T, r = series(rec, site_lon, site_lat, r_out_km, dt_s, substeps, **prof)
        n_band += int((np.abs(r - r_out_km) <= BAND_KM).sum())
        any_ = inside.any(axis=1)
        for i, m in enumerate(window_samples):
            A[i, :, s] = np.where(any_, window_max(T, m), np.nan)
    return A, n_band


def counts(A, groups, n_groups, thresholds):
    """[n_site][n_groups][n_window][n_bin] int32 from A [n_window][n_site][n_trk]: storms of each group with A >= thr."""
    thr = np.asarray(thresholds, float)
    with np.errstate(invalid='ignore'):
        hit = A[:, :, :, None] >= thr
    out = np.zeros((A.shape[1], n_groups, A.shape[0], thr.size), np.int32)
    for g in range(n_groups):
        out[:, g] = hit[:, :, np.asarray(groups) == g].sum(axis=2).transpose(1, 0, 2)
    return out


def near_threshold(A, thresholds):
    """[n_window][n_site][n_trk]: the value is within the tolerance of a threshold, so its count may differ."""
    thr = np.asarray(thresholds, float)
    with np.errstate(invalid='ignore'):
        return (np.abs(A[..., None] - thr) <= TOL_ABS + TOL_REL * np.abs(thr)).any(axis=-1)


def close_to(got, want, scale):
    """|got - want| <= TOL_ABS + TOL_REL |scale|, NaN equal to NaN."""
    with np.errstate(invalid='ignore'):
        return (np.abs(got - want) <= TOL_ABS + TOL_REL * np.abs(scale)) | (np.isnan(got) & np.isnan(want))
