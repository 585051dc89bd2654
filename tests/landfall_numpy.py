"""NumPy restatement of the landfall contract (include/tcrisk_hip.h, "landfall" section; tropical_cyclone_risk_amd/landfall.py).

Land node: land >= 1 (NaN: water).  A sample's cell by comparisons: i = the last node <= x (0 below the grid), node i + 1 counts
iff it exists (or the grid is periodic: node 0) and lon_i < x; the same for lat (never periodic).  A periodic grid
(lon[-1] - lon[0] + (lon[1] - lon[0]) == 360) reduces x first: t = fmod(x - lon0, 360), t += 360 where t < 0, x = lon0 + t, and
lon0 where that is >= lon0 + 360.  Over land: every counted node is land.  Event: a live sample over land whose previous live
sample is not; v_landfall = vmax at that previous sample, v_inland = vmax at the event.
"""
import numpy as np


def periodic(lon):
    lon = np.asarray(lon, float)
    return bool(lon[-1] - lon[0] + (lon[1] - lon[0]) == 360.0)


def reduce_lon(x, lon):
    lon0 = float(lon[0])
    with np.errstate(invalid='ignore'):
        t = np.fmod(np.asarray(x, float) - lon0, 360.0)
        t = np.where(t < 0.0, t + 360.0, t)
        r = lon0 + t
        return np.where(r >= lon0 + 360.0, lon0, r)


def cell(xs, x, wrap):
    """(i, two): the last node <= x (0 below the grid or for NaN) and whether the next node has a nonzero weight."""
    xs = np.asarray(xs, float)
    n = xs.size
    x = np.asarray(x, float)
    i = np.clip(np.searchsorted(xs, x, side='right') - 1, 0, n - 1)
    i = np.where(np.isnan(x), 0, i)
    with np.errstate(invalid='ignore'):
        two = ((i + 1 < n) | wrap) & (xs[i] < x)
    return i, two


def over_land(x, y, lon, lat, land):
    """The land decision of every (x, y) sample (any shape); NaN samples give False."""
    lon, lat = np.asarray(lon, float), np.asarray(lat, float)
    with np.errstate(invalid='ignore'):
        node = np.asarray(land, float) >= 1.0
    wrap = periodic(lon)
    x, y = np.asarray(x, float), np.asarray(y, float)
    if wrap:
        x = reduce_lon(x, lon)
    i, tx = cell(lon, x, wrap)
    j, ty = cell(lat, y, False)
    i1 = np.where(i + 1 < lon.size, i + 1, 0)
    j1 = np.minimum(j + 1, lat.size - 1)
    out = node[j, i] & (~tx | node[j, i1]) & (~ty | node[j1, i]) & (~(tx & ty) | node[j1, i1])
    return out & ~np.isnan(x) & ~np.isnan(y)


def flags(lon_t, lat_t, lon, lat, land):
    """[n_trk][n_t] uint8: 0 water, 1 land, 2 not live."""
    live = ~np.isnan(lon_t) & ~np.isnan(lat_t)
    ol = over_land(lon_t, lat_t, lon, lat, land)
    return np.where(live, ol.astype(np.uint8), np.uint8(2)).astype(np.uint8)


def landfalls(lon_t, lat_t, vmax, lon, lat, land):
    """dict(n_landfall [n_trk] int32, k [n_trk][m] int32 (-1 padded), lon, lat, v_landfall, v_inland [n_trk][m] (NaN padded),
    flags [n_trk][n_t]) with m = max(n_landfall)."""
    lon_t, lat_t, vmax = (np.asarray(a, float) for a in (lon_t, lat_t, vmax))
    n_trk, n_t = lon_t.shape
    live = ~np.isnan(lon_t) & ~np.isnan(lat_t)
    ol = over_land(lon_t, lat_t, lon, lat, land) & live
    # previous live sample of every sample (-1: none)
    idx = np.where(live, np.arange(n_t)[None, :], -1)
    last = np.maximum.accumulate(idx, axis=1)
    prev = np.concatenate([np.full((n_trk, 1), -1), last[:, :-1]], axis=1)
    rows = np.arange(n_trk)[:, None]
    prev_land = ol[rows, np.maximum(prev, 0)]
    ev = ol & (prev >= 0) & ~prev_land
    n = ev.sum(axis=1).astype(np.int32)
    m = int(n.max()) if n_trk else 0
    out = dict(n_landfall=n, k=np.full((n_trk, m), -1, np.int32), flags=np.where(live, ol.astype(np.uint8), np.uint8(2)))
    for key in ('lon', 'lat', 'v_landfall', 'v_inland'):
        out[key] = np.full((n_trk, m), np.nan)
    s, k = np.nonzero(ev)                                    # row-major: every storm's events in order
    if s.size:
        slot = np.arange(s.size) - np.concatenate([[0], np.cumsum(n)[:-1]])[s]
        out['k'][s, slot] = k
        out['lon'][s, slot] = lon_t[s, k]
        out['lat'][s, slot] = lat_t[s, k]
        out['v_landfall'][s, slot] = vmax[s, prev[s, k]]
        out['v_inland'][s, slot] = vmax[s, k]
    return out


def brute_force_over_land(x, y, lon, lat, land):
    """Rule 2 node by node: the hat function of node i is nonzero on (lon_{i-1}, lon_{i+1}) (the first / last node also below /
    above the grid, where FITPACK clamps; across the wrap on a periodic grid); a sample is over land iff every node whose lon hat
    and lat hat are both nonzero is land.  For small grids and few points."""
    lon, lat = np.asarray(lon, float), np.asarray(lat, float)
    node = np.asarray(land, float) >= 1.0
    wrap = periodic(lon)

    def hats(xs, v, wrap_):
        n = xs.size
        w = np.zeros(n, bool)
        if np.isnan(v):
            w[0] = True
            return w
        if not wrap_:
            v = min(max(v, xs[0]), xs[-1])
        for i in range(n):
            lo = xs[i - 1] if i > 0 else (xs[-1] - 360.0 if wrap_ else -np.inf)
            hi = xs[i + 1] if i + 1 < n else (xs[0] + 360.0 if wrap_ else np.inf)
            w[i] = lo < v < hi or v == xs[i]
        if wrap_:                                            # node 0 seen from the wrap cell [lon[-1], lon0 + 360)
            w[0] = w[0] or v > xs[-1]
        return w
    out = np.zeros(np.shape(x), bool)
    for n_, (a, b) in enumerate(zip(np.ravel(x), np.ravel(y))):
        if np.isnan(a) or np.isnan(b):
            continue
        if wrap:
            a = float(reduce_lon(a, lon))
        wx, wy = hats(lon, a, wrap), hats(lat, b, False)
        out.flat[n_] = bool(node[np.ix_(wy, wx)].all())
    return out
