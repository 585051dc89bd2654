"""NumPy restatement of the directional-wind contract (include/tcrisk_hip.h "directional wind",
tropical_cyclone_risk_amd/directional.py), on the wind footprint's restatement (tests/windfield_numpy.py): its samples, its
distance, its profile, its r_out band and its tolerance.  The wind vector is re-formed as WN.wind forms it, and the direction it
blows from is theta = atan2(-w_e, -w_n), written with np.arctan2 rather than the kernel's half-plane tests.

A pair is ambiguous when its distance is within WN.BAND_KM of r_out (either inclusion decision is accepted), when its bearing is
within BOUNDARY_RAD of a sector boundary (either neighbouring sector is accepted) or when its distance is below NEAR_KM (any sector
is accepted).  The last two: the bearing's components carry a few 1e-16 of absolute rounding, and at 1 m from the centre the
centre-to-site vector is 1.6e-7 rad long, so the direction is good to about 2e-9 there and better farther out.
"""
import numpy as np

from tests import windfield_numpy as WN

BOUNDARY_RAD = 1e-8
NEAR_KM = 1e-3


def wind_vector(site_lon, site_lat, lon, lat, v, rm_km, ae, an, c):
    """(w_e, w_n, |w|, r km) of samples (lon, lat, v, rm, A) at sites, broadcast: the vector whose length WN.wind returns."""
    r = WN.haversine_km(lon, lat, site_lon, site_lat)
    V = WN.profile(r, rm_km, v, lat, c)
    ps, pc = np.deg2rad(site_lat), np.deg2rad(lat)
    dl = np.deg2rad(site_lon) - np.deg2rad(lon)
    e = np.cos(ps) * np.sin(dl)
    n = np.cos(pc) * np.sin(ps) - np.sin(pc) * np.cos(ps) * np.cos(dl)
    den = np.hypot(e, n)
    with np.errstate(divide='ignore', invalid='ignore'):
        de, dn = np.where(den > 0, e / den, 0.0), np.where(den > 0, n / den, 0.0)
        h = np.where(np.asarray(lat) >= 0, 1.0, -1.0)
        q = np.where(v > 0, V / v, 0.0)
    we, wn = V * (-h * dn) + q * ae, V * (h * de) + q * an
    live = (v > 0) & (den > 0)
    we, wn = np.where(live, we, 0.0), np.where(live, wn, 0.0)
    return we, wn, np.hypot(we, wn), r


def from_deg(we, wn):
    """The direction the wind (we, wn) blows from: degrees clockwise from north in [0, 360)."""
    return np.rad2deg(np.arctan2(-we, -wn)) % 360.0


def sector_of(theta_deg, n_sector, sector0_deg):
    """(sector, the other sector the bearing is within BOUNDARY_RAD of, or -1)."""
    width = 360.0 / n_sector
    x = ((np.asarray(theta_deg, float) - sector0_deg) % 360.0) / width + 0.5
    k = np.floor(x).astype(np.int64) % n_sector
    frac = x - np.floor(x)
    tol = np.rad2deg(BOUNDARY_RAD) / width
    other = np.where(frac <= tol, (k - 1) % n_sector, np.where(1.0 - frac <= tol, (k + 1) % n_sector, -1))
    return k, np.where(n_sector > 1, other, -1)


def directional(recs, site_lon, site_lat, r_out_km, c, n_sector, sector0_deg):
    """recs: WN.samples(...).  Returns (lo, amb, inc_any, inc_sure): lo [n_sector][n_site][n_trk] the max of |w| over the surely
    included pairs that are surely in the sector, 0.0 where there is none but a pair of the storm is surely included, NaN where
    none is; amb {(site, storm): (winds [n], may [n][n_sector] the sectors each ambiguous pair might fall in)}; inc_any /
    inc_sure [n_site][n_trk]: some pair is surely or ambiguously / surely included."""
    site_lon, site_lat = np.asarray(site_lon, float), np.asarray(site_lat, float)
    n_site, n_trk = site_lon.size, len(recs)
    lo = np.full((n_sector, n_site, n_trk), np.nan)
    inc_any = np.zeros((n_site, n_trk), bool)
    inc_sure = np.zeros((n_site, n_trk), bool)
    amb = {}
    for s, rec in enumerate(recs):
        if rec is None:
            continue
        we, wn, w, r = wind_vector(site_lon[:, None], site_lat[:, None], *[x[None, :] for x in rec], c)
        band = np.abs(r - r_out_km) <= WN.BAND_KM
        inside = (r <= r_out_km) & ~band
        inc_any[:, s] = (inside | band).any(axis=1)
        inc_sure[:, s] = inside.any(axis=1)
        k, other = sector_of(from_deg(we, wn), n_sector, sector0_deg)
        blows = w > 0
        near = blows & (r < NEAR_KM) & (n_sector > 1)
        edge = blows & (other >= 0)
        unsure = band | (inside & (near | edge))        # (a band pair without wind still decides between NaN and 0.0)
        sure = inside & blows & ~unsure
        for j in range(n_sector):
            m = np.where(sure & (k == j), w, 0.0).max(axis=1)
            lo[j, :, s] = np.where(inc_sure[:, s], m, np.nan)
        for i in np.nonzero(unsure.any(axis=1))[0]:
            idx = np.nonzero(unsure[i])[0]
            may = np.zeros((idx.size, n_sector), bool)
            may[np.arange(idx.size), k[i, idx]] = True
            has = other[i, idx] >= 0
            may[np.nonzero(has)[0], other[i, idx][has]] = True
            may[near[i, idx]] = True
            amb[(int(i), s)] = (w[i, idx], may)
    return lo, amb, inc_any, inc_sure


def ambiguous_cells(amb, shape):
    """[n_site][n_trk]: the (site, storm) has an ambiguous pair."""
    out = np.zeros(shape, bool)
    for i, s in amb:
        out[i, s] = True
    return out


def allowed(got, lo, amb, inc_any, inc_sure):
    """True where got[sector][site][storm] is what the restatement gives for SOME choice of the ambiguous decisions: close to
    lo, or to an ambiguous wind above lo that might fall in the sector; NaN in every sector where no pair is surely included and
    the ambiguous ones are left out; NaN nowhere a pair is surely included, and everywhere none possibly is."""
    nan = np.isnan(got)
    maybe = inc_any & ~inc_sure                 # included only through pairs in the r_out band: NaN in every sector, or in none
    ok = WN.close(got, lo) | (maybe[None] & ~nan.any(axis=0)[None] & WN.close(got, 0.0))
    for (i, s), (winds, may) in amb.items():
        base = np.where(np.isnan(lo[:, i, s]), 0.0, lo[:, i, s])
        for w, m in zip(winds, may):
            for j in np.nonzero(m)[0]:
                if not nan[j, i, s] and w > base[j] and WN.close(got[j, i, s], w):
                    ok[j, i, s] = True
    mixed = nan.any(axis=0) & ~nan.all(axis=0)
    return ok & ~mixed[None] & ~(nan & inc_sure[None]) & ~(~nan & ~inc_any[None])


def counts(planes, groups, n_groups, thresholds):
    """[n_site][n_groups][n_sector][n_bin] int32 from planes [n_sector][n_site][n_trk]: storms of each group with peak >= thr
    (a NaN counts nowhere)."""
    thr = np.asarray(thresholds, float)
    with np.errstate(invalid='ignore'):
        hit = planes[:, :, :, None] >= thr                              # [n_sector][n_site][n_trk][n_bin]
    out = np.zeros((planes.shape[1], n_groups, planes.shape[0], thr.size), np.int32)
    for g in range(n_groups):
        out[:, g] = hit[:, :, np.asarray(groups) == g].sum(axis=2).transpose(1, 0, 2)
    return out
