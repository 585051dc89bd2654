"""NumPy restatement of the wind-duration contract (include/tcrisk_hip.h "wind duration", tropical_cyclone_risk_amd/duration.py),
on the wind footprint's restatement (tests/windfield_numpy.py): its samples, its wind, its r_out band and its tolerance.

Record q of a storm's n_rec records carries the integer half-weight 2, or 1 for q = 0 and q = n_rec - 1.  Per (level, site, storm)
the half-weights of the records that are within r_out of the site and whose wind is >= the level add up to H; the hours are
H u with u = dt_s / (7200 substeps).  A record is ambiguous when its distance is within BAND_KM of r_out or its wind within
TOL_ABS + TOL_REL level of the level: either decision is accepted for it, so the restatement gives bounds lo <= H <= hi.
"""
import numpy as np

from tests import windfield_numpy as WN


def unit_hours(dt_s, substeps):
    """u: the hours per half-weight."""
    return dt_s / (7200.0 * substeps)


def half_weights(n_rec):
    h = np.full(n_rec, 2, dtype=np.int64)
    h[0] = h[-1] = 1
    return h


def duration(recs, site_lon, site_lat, r_out_km, c, levels):
    """recs: WN.samples(...).  Returns (lo, hi, n_amb, included_any, included_sure): lo, hi [n_level][n_site][n_trk] int64, the
    half-weights of the records surely included and surely at or above the level, and those plus the ambiguous records';
    n_amb [n_level][n_site][n_trk] the number of ambiguous records; included_any / included_sure [n_site][n_trk]: some record is
    surely or ambiguously / surely included."""
    site_lon, site_lat = np.asarray(site_lon, float), np.asarray(site_lat, float)
    levels = np.asarray(levels, float).reshape(-1)
    n_site, n_trk = site_lon.size, len(recs)
    lo = np.zeros((levels.size, n_site, n_trk), np.int64)
    hi = np.zeros_like(lo)
    n_amb = np.zeros_like(lo)
    inc_any = np.zeros((n_site, n_trk), bool)
    inc_sure = np.zeros((n_site, n_trk), bool)
    for s, rec in enumerate(recs):
        if rec is None:
            continue
        w, r = WN.wind(site_lon[:, None], site_lat[:, None], *[x[None, :] for x in rec], c)
        h = half_weights(rec.shape[1])[None, :]
        band = np.abs(r - r_out_km) <= WN.BAND_KM
        inside = (r <= r_out_km) & ~band
        inc_any[:, s] = (inside | band).any(axis=1)
        inc_sure[:, s] = inside.any(axis=1)
        for l, lev in enumerate(levels):
            near = np.abs(w - lev) <= WN.TOL_ABS + WN.TOL_REL * lev
            amb = band | near
            lo[l, :, s] = ((inside & (w >= lev) & ~amb) * h).sum(axis=1)
            hi[l, :, s] = lo[l, :, s] + (amb * h).sum(axis=1)
            n_amb[l, :, s] = amb.sum(axis=1)
    return lo, hi, n_amb, inc_any, inc_sure


def hours(H, included, u):
    """[...][n_site][n_trk] fp64: (double)H u, NaN where not included."""
    return np.where(included, H.astype(np.float64) * u, np.nan)


def counts(site_hours, groups, n_groups, thresholds):
    """[n_site][n_groups][n_level][n_bin] int32 from site_hours [n_level][n_site][n_trk]: storms of each group with hours >= thr."""
    thr = np.asarray(thresholds, float)
    with np.errstate(invalid='ignore'):
        hit = site_hours[:, :, :, None] >= thr                          # [n_level][n_site][n_trk][n_bin]
    out = np.zeros((site_hours.shape[1], n_groups, site_hours.shape[0], thr.size), np.int32)
    for g in range(n_groups):
        out[:, g] = hit[:, :, np.asarray(groups) == g].sum(axis=2).transpose(1, 0, 2)
    return out


def half_steps(H, groups, n_groups):
    """[n_site][n_groups][n_level] int64 from H [n_level][n_site][n_trk]."""
    out = np.zeros((H.shape[1], n_groups, H.shape[0]), np.int64)
    for g in range(n_groups):
        out[:, g] = H[:, :, np.asarray(groups) == g].sum(axis=2).T
    return out
