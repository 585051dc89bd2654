"""Generate tests/golden/landfall_golden.npz: the reference's own land decision on the reference's land mask.

    python tests/golden/make_golden_landfall.py      (reference checkout: ref_harness.REF)

The interpolator is built as `geo.read_land` builds it (intensity/geo.py:23-34): the reference's intensity/data/land.nc (the same
bytes as tests/golden/ref_land.nc), cropped by the reference's own `TC_Basin(b).transform_global_field`, handed to
RectBivariateSpline(kx=1, ky=1); `_get_over_land` tests `ev(lon, lat) == 1` (coupled_fast.py:35-38).  Recorded for the NA and GL
basins: `ev` at
  - every live sample of tests/golden/tracks_NA_res0125.npz (traj[:, 0] = lon, traj[:, 1] = lat; the points are not stored),
  - random points within 0.25 degrees of coastline nodes (land nodes with a water neighbour), all over the globe,
  - points exactly on nodes, on lon grid lines and on lat grid lines.
Also stored: each basin's crop (lon / lat range of the cropped grid).  Data only.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from tests.golden import ref_harness as H            # noqa: E402
from tropical_cyclone_risk_amd.fields import _Dataset  # noqa: E402


def extra_points(lon, lat, land, rng):
    node = land >= 1
    coast = node & ~(np.roll(node, 1, 1) & np.roll(node, -1, 1) & np.roll(node, 1, 0) & np.roll(node, -1, 0))
    j, i = np.nonzero(coast)
    pick = rng.choice(j.size, 4000, replace=False)
    cx = lon[i[pick]] + rng.uniform(-0.25, 0.25, pick.size)
    cy = lat[j[pick]] + rng.uniform(-0.25, 0.25, pick.size)
    cx = np.mod(cx, 360.0)
    # exactly on nodes (half of them coastal), on lon lines, on lat lines
    nj = np.concatenate([j[rng.choice(j.size, 300)], rng.integers(0, lat.size, 300)])
    ni = np.concatenate([i[rng.choice(i.size, 300)], rng.integers(0, lon.size, 300)])
    k = rng.choice(j.size, 1000)
    lx, ly = lon[i[k[:500]]], lat[j[k[:500]]] + rng.uniform(-0.125, 0.125, 500)
    gx, gy = lon[i[k[500:]]] + rng.uniform(-0.125, 0.125, 500), lat[j[k[500:]]]
    px = np.concatenate([cx, lon[ni], lx, np.mod(gx, 360.0)])
    py = np.concatenate([cy, lat[nj], ly, gy])
    kind = np.concatenate([np.zeros(cx.size), np.ones(ni.size), np.full(lx.size, 2), np.full(gx.size, 3)]).astype(np.int8)
    return px, py, kind


def main():
    from scipy.interpolate import RectBivariateSpline
    d = _Dataset(os.path.join(H.REF, 'intensity', 'data', 'land.nc'))    # (before the reference import stubs xarray)
    ref = H.import_reference()
    lon, lat = np.asarray(d['lon'], float), np.asarray(d['lat'], float)
    land_raw = np.asarray(d.vars['land'])
    land = np.asarray(land_raw, float)
    assert lat[1] > lat[0]
    tr = np.load(os.path.join(HERE, 'tracks_NA_res0125.npz'))['traj']
    tx, ty = tr[:, 0].ravel(), tr[:, 1].ravel()
    live = ~np.isnan(tx) & ~np.isnan(ty)
    tx, ty = tx[live], ty[live]
    px, py, kind = extra_points(lon, lat, land, np.random.default_rng(606))
    out = dict(px=px, py=py, kind=kind, n_track_points=tx.size)
    warnings.simplefilter('ignore')
    for b in ('NA', 'GL'):
        basin = ref.basins.TC_Basin(b)
        lon_b, lat_b, land_b = basin.transform_global_field(lon, lat, land_raw)
        f = RectBivariateSpline(lon_b, lat_b, land_b.T, kx=1, ky=1)
        out['ev_track_%s' % b] = f.ev(tx, ty)
        out['ev_%s' % b] = f.ev(px, py)
        out['crop_%s' % b] = np.array([lon_b[0], lon_b[-1], lat_b[0], lat_b[-1]])
        ev = np.concatenate([out['ev_track_%s' % b], out['ev_%s' % b]])
        print('%s: crop lon %g..%g lat %g..%g; %d points, %d with ev == 1, %d in 1 - 1e-12 <= ev < 1'
              % (b, lon_b[0], lon_b[-1], lat_b[0], lat_b[-1], ev.size, int((ev == 1).sum()), int(((ev >= 1 - 1e-12) & (ev < 1)).sum())))
    fn = os.path.join(HERE, 'landfall_golden.npz')
    np.savez_compressed(fn, **out)
    print('%s: %d bytes' % (fn, os.path.getsize(fn)))


if __name__ == '__main__':
    main()
