"""Generate tests/golden/hazard_golden.npz: the reference notebook's site analysis on the reference's own tracks.

    python tests/golden/make_golden_hazard.py      (reference checkout: ref_harness.REF)

The notebook (notebooks/sample_analysis.ipynb) cell that defines `haversine` is executed as it stands; its
`vmax_trks.where(dists <= R).max(dim='time')` is applied with np.where + np.nanmax (the same NaN-skipping semantics; xarray is
not needed) and its exceedance loop as written there.  Tracks: tests/golden/tracks_NA.npz and tracks_GL.npz (traj[:, 0] = lon,
traj[:, 1] = lat; vmax).  Storms are spread over 5 fake years in an unsorted order.
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ref_harness import REF  # noqa: E402
from tests.hazard_numpy import offset_point  # noqa: E402
R_KM = 100.0
THRESHOLDS = np.arange(10, 81, 5)


def notebook_haversine(ref):
    nb = json.load(open(os.path.join(ref, 'notebooks', 'sample_analysis.ipynb')))
    for c in nb['cells']:
        src = ''.join(c['source'])
        if c['cell_type'] == 'code' and 'def haversine' in src:
            ns = {'np': np}
            exec(src, ns)
            return ns['haversine'], ns['clon'], ns['clat']
    raise RuntimeError('no haversine cell in the notebook')


def tracks():
    lon, lat, vmax = [], [], []
    for b in ('NA', 'GL'):
        d = np.load(os.path.join(HERE, 'tracks_%s.npz' % b))
        lon.append(d['traj'][:, 0]); lat.append(d['traj'][:, 1]); vmax.append(d['vmax'])
    return np.concatenate(lon), np.concatenate(lat), np.concatenate(vmax)


def main(ref):
    haversine, clon, clat = notebook_haversine(ref)
    lon, lat, vmax = tracks()
    rng = np.random.default_rng(2024)
    live = np.argwhere(~np.isnan(lon))
    pick = live[rng.choice(len(live), 24, replace=False)]
    near_lon, near_lat = offset_point(lon[pick[:, 0], pick[:, 1]], lat[pick[:, 0], pick[:, 1]],
                                      rng.uniform(0.3, 1.5, len(pick)) * R_KM, rng.uniform(0, 2 * np.pi, len(pick)))
    # the same sites in the other convention (tracks are 0..360: near sites are there, their copies in -180..180)
    other = np.where(near_lon > 180, near_lon - 360, near_lon + 360)
    gl = np.argwhere(np.abs(lon - 180) < 5)
    dl = [float(lon[tuple(gl[0])]) - 0.2, float(lat[tuple(gl[0])])] if len(gl) else [179.9, 20.0]
    site_lon = np.concatenate([[clon], near_lon, other, [dl[0], -180.0 + (dl[0] - 180.0)]])
    site_lat = np.concatenate([[clat], near_lat, near_lat, [dl[1], dl[1]]])
    groups = rng.integers(0, 5, lon.shape[0])

    smax = np.empty((site_lon.size, lon.shape[0]))
    counts = np.zeros((site_lon.size, 5, THRESHOLDS.size), dtype=np.int32)
    for i in range(site_lon.size):
        dists = haversine(site_lon[i], site_lat[i], lon, lat)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            vmax_at_poi = np.nanmax(np.where(dists <= R_KM, vmax, np.nan), axis=1)
        smax[i] = vmax_at_poi
        for g in range(5):
            flat = vmax_at_poi[groups == g]
            for k in range(len(THRESHOLDS)):
                counts[i, g, k] = np.sum(flat >= THRESHOLDS[k])
    total_years = 5
    exceedance_count = counts.sum(axis=1).astype(float)
    with np.errstate(divide='ignore'):
        rp = total_years / exceedance_count
    np.savez_compressed(os.path.join(HERE, 'hazard_golden.npz'), site_lon=site_lon, site_lat=site_lat, groups=groups,
                        radius_km=R_KM, thresholds=THRESHOLDS.astype(float), site_max=smax, counts=counts, return_period=rp,
                        total_years=total_years, tracks=np.array(['tracks_NA.npz', 'tracks_GL.npz']))
    print('hazard_golden.npz: %d sites x %d storms, %d (site, storm) pairs with a sample within %g km'
          % (site_lon.size, lon.shape[0], int(np.sum(~np.isnan(smax))), R_KM))


if __name__ == '__main__':
    main(REF)
