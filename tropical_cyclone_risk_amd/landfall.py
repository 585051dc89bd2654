"""Landfall: where storms come ashore, how strong they are then, and the return periods of landfall intensity.

A landfall is the sample at which the model's own land decision (``f_land.ev(lon, lat) == 1`` on the bilinear interpolant of
``intensity/data/land.nc``, coupled_fast.py:35-38) goes from sea to land, with that decision taken on the grid nodes so that the
bilinear sum's rounding does not make spurious landfalls inland (``csrc/tcr_landfall.hip``; the contract is in the header's
"landfall" section and DESIGN.md section 8, f-6).  Per event: the sample index, its lon / lat (the first land sample), the
intensity at the last water sample (``v_landfall``) and at the first land sample (``v_inland``).

On top of the events: per (file, year) group, the storms whose first-landfall (or largest landfall) intensity is ``>= v``,
basin-wide and in lon / lat boxes; near sites, the site-hazard analysis (``hazard.site_hazard``) run on the event locations.
Return periods are ``total_years / count``.  Hourly samples can step over a land strip narrower than an hour's motion: such a
crossing is not a landfall.

    python -m tropical_cyclone_risk_amd.landfall TRACKS.nc [...] --land land.nc --region FL=-88:-79,24:31 --out landfall.npz
"""
import argparse
import ctypes as C
import sys
import weakref

import numpy as np

from . import _lib, analysis, hazard
from .analysis import DEFAULT_THRESHOLDS, to_numpy as _np

EVENT_FIELDS = ('lon', 'lat', 'v_landfall', 'v_inland')
_FIRST_CAPACITY = 8


class LandGrid:
    """A land grid for the land decision: lon [nlon], lat [nlat] ascending (a north-to-south lat is flipped, as
    `fields._ascending_lat` does), land [nlat][nlon] (a node is land iff land >= 1; NaN is water)."""

    def __init__(self, lon, lat, land):
        from .fields import _ascending_lat
        lon = np.ascontiguousarray(np.asarray(lon, dtype=np.float64).reshape(-1))
        land = np.asarray(land, dtype=np.float64)
        lat, land = _ascending_lat(np.asarray(lat, dtype=np.float64).reshape(-1), land)
        if land.shape != (lat.size, lon.size):
            raise ValueError('land must be [nlat][nlon] = [%d][%d], got %s' % (lat.size, lon.size, land.shape))
        self.lon, self.lat, self.land = lon, np.ascontiguousarray(lat), np.ascontiguousarray(land)

    @property
    def periodic(self):
        """The grid covers the circle: lon[-1] - lon[0] + (lon[1] - lon[0]) == 360 exactly."""
        x = self.lon
        return x.size >= 2 and bool(x[-1] - x[0] + (x[1] - x[0]) == 360.0)


def read_land(fn):
    """The reference's land.nc schema (variables lon, lat, land) through `fields._Dataset` (NetCDF-3 or NetCDF-4)."""
    from .fields import _Dataset
    d = _Dataset(fn)
    return LandGrid(d['lon'], d['lat'], d['land'])


_uploaded = weakref.WeakKeyDictionary()          # engine -> the LandGrid its context holds


def _upload(ctx, grid, engine):
    if engine is not None and _uploaded.get(engine) is grid:
        return
    g = _lib.LandGrid(nlon=grid.lon.size, nlat=grid.lat.size, lon=grid.lon.ctypes.data, lat=grid.lat.ctypes.data,
                      land=grid.land.ctypes.data)
    ctx.check(ctx.L.tcr_land_upload(ctx.h, C.byref(g)))
    if engine is not None:
        _uploaded[engine] = grid


def detect_landfalls(lon, lat, vmax, land_grid, engine=None, device=0, return_flags=False):
    """Landfall events of every storm.

    lon, lat, vmax: [n_trk][n_t] fp64 (the track file's lon_trks, lat_trks, vmax_trks; NaN past a track's end), NumPy arrays or
    torch tensors on the GPU (then everything stays there).  land_grid: a `LandGrid` (`read_land`) or (lon, lat, land).
    Returns a dict of the type and device of ``lon``: ``n_landfall`` [n_trk] int32 (every event), the event planes ``k``
    (int32, -1 padded) and ``lon``, ``lat``, ``v_landfall``, ``v_inland`` (NaN padded), all [n_trk][max(n_landfall)], and with
    ``return_flags`` ``flags`` [n_trk][n_t] uint8 (0 water, 1 land, 2 not live).  The first event of a storm is column 0.
    ``engine``: a TCEngine whose context is used (None: one is opened for the call).
    """
    grid = land_grid if isinstance(land_grid, LandGrid) else LandGrid(*land_grid)
    (lon, lat, vmax), fl = analysis.as_planes((lon, lat, vmax), 'lon, lat and vmax')
    lon, lat, vmax = (fl.contiguous(a) for a in (lon, lat, vmax))
    n_trk, n_t = int(lon.shape[0]), int(lon.shape[1])
    if n_t < 1:
        raise ValueError('the tracks need at least one sample')
    new, ptr = fl.new, fl.ptr
    trk = _lib.HazardTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=ptr(lon), lat=ptr(lat), vmax=ptr(vmax), n_group=0,
                            group_off=None)
    n_lf = new((n_trk,), 'i4')
    flags = new((n_trk, n_t), 'u1') if return_flags else None
    with fl.context(engine, device) as ctx:
        _upload(ctx, grid, engine)

        def run(cap, flag_buf):
            k = new((n_trk, cap), 'i4')
            planes = [new((n_trk, cap), 'f8') for _ in EVENT_FIELDS]
            if n_trk:
                ctx.call('tcr_landfall', C.byref(trk), cap, ptr(n_lf), ptr(k), *[ptr(p) for p in planes],
                         ptr(flag_buf) if flag_buf is not None else None)
            return k, planes
        k, planes = run(_FIRST_CAPACITY, flags)
        n_max = int(n_lf.max()) if n_trk else 0             # (a device tensor: waits for the call)
        if n_max > _FIRST_CAPACITY:
            k, planes = run(n_max, None)
    res = dict(n_landfall=n_lf, k=k[:, :n_max])
    for name, p in zip(EVENT_FIELDS, planes):
        res[name] = p[:, :n_max]
    if return_flags:
        res['flags'] = flags
    return res


# ---------------------------------------------------------------------------------------------------------- aggregates
def in_box(lon, lat, box):
    """lon0 <= lon <= lon1 along the circle (the box may cross the dateline; either longitude convention) and
    lat0 <= lat <= lat1.  box = (lon0, lon1, lat0, lat1).  NaN is outside."""
    lon0, lon1, lat0, lat1 = (float(b) for b in box)
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        if lon1 - lon0 >= 360.0:
            along = ~np.isnan(lon)
        else:
            along = np.mod(lon - lon0, 360.0) <= np.mod(lon1 - lon0, 360.0)
        return along & (lat >= lat0) & (lat <= lat1)


def _storm_counts(v_first, v_max, hit, groups, n_groups, thr):
    """[n_groups][n_bin] storms with first / max intensity >= thr, and [n_groups] storms with an event (hit)."""
    with np.errstate(invalid='ignore'):
        ge_first = v_first[:, None] >= thr[None, :]
        ge_max = v_max[:, None] >= thr[None, :]
    first = np.zeros((n_groups, thr.size), dtype=np.int64)
    mx = np.zeros((n_groups, thr.size), dtype=np.int64)
    np.add.at(first, groups, ge_first.astype(np.int64))
    np.add.at(mx, groups, ge_max.astype(np.int64))
    return first, mx, np.bincount(groups, weights=hit.astype(np.int64), minlength=n_groups).astype(np.int64)


def _first_and_max(v, sel):
    """Per storm: v at the first selected event and the NaN-skipping max of v over the selected events (NaN: none)."""
    n_trk = v.shape[0]
    has = sel.any(axis=1)
    first = np.full(n_trk, np.nan)
    if v.shape[1]:
        first[has] = v[has, np.argmax(sel[has], axis=1)]
    vm = np.where(sel, v, np.nan)
    mx = np.full(n_trk, np.nan)
    ok = (sel & ~np.isnan(v)).any(axis=1)
    if ok.any():
        mx[ok] = np.nanmax(vm[ok], axis=1)
    return first, mx, has


def landfall_counts(events, groups, thresholds=DEFAULT_THRESHOLDS, regions=None, n_groups=None):
    """Exceedance counts of landfall intensity per group.

    events: the dict of `detect_landfalls`; groups: [n_trk] integer group of every storm (a (file, year) of
    `hazard.load_groups`).  Returns ``first`` [n_groups][n_bin] (storms whose first landfall's v_landfall >= threshold), ``max``
    (the same for the storm's largest v_landfall), ``n_storms`` [n_groups] (storms with a landfall) and ``thresholds``.  regions:
    {name: (lon0, lon1, lat0, lat1)} (or a list of (name, box)): ``region_first``, ``region_max`` [n_region][n_groups][n_bin] and
    ``region_n_storms`` [n_region][n_groups] restricted to the events inside each box, and ``region_names``, ``region_box``.
    NaN intensities never reach a threshold.  ``hazard.return_periods`` turns counts into return periods."""
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    v = _np(events['v_landfall']).astype(np.float64)
    elon, elat = _np(events['lon']).astype(np.float64), _np(events['lat']).astype(np.float64)
    live = _np(events['k']) >= 0
    g, n_groups = analysis.group_index(groups, v.shape[0], n_groups)
    first, mx, has = _first_and_max(v, live)
    c_first, c_max, n_st = _storm_counts(first, mx, has, g, n_groups, thr)
    res = dict(first=c_first, max=c_max, n_storms=n_st, thresholds=thr)
    if regions is not None:
        items = list(regions.items()) if isinstance(regions, dict) else list(regions)
        rf, rm, rn = [], [], []
        for _, box in items:
            f, m, h = _first_and_max(v, live & in_box(elon, elat, box))
            a, b, c = _storm_counts(f, m, h, g, n_groups, thr)
            rf.append(a); rm.append(b); rn.append(c)
        shape = (0, n_groups, thr.size)
        res.update(region_names=np.array([str(n) for n, _ in items]),
                   region_box=np.array([[float(x) for x in b] for _, b in items]).reshape(-1, 4),
                   region_first=np.array(rf).reshape(shape) if not rf else np.array(rf),
                   region_max=np.array(rm).reshape(shape) if not rm else np.array(rm),
                   region_n_storms=np.array(rn).reshape(0, n_groups) if not rn else np.array(rn))
    return res


def landfall_site_hazard(events, groups, site_lon, site_lat, radius_km=100., thresholds=DEFAULT_THRESHOLDS, return_max=False,
                         engine=None, device=0, n_groups=None):
    """`hazard.site_hazard` on the landfall events: per site and storm the NaN-skipping max of v_landfall over the storm's
    events within radius_km of the site (the notebook's haversine), and the exceedance counts per group.  Runs on the GPU; with
    device tensors as events everything stays there."""
    planes = [events['lon'], events['lat'], events['v_landfall']]
    if int(planes[0].shape[1]) == 0:                       # no storm made landfall: one empty (NaN) event column
        if analysis.is_tensor(planes[0]):
            import torch
            planes = [torch.full((int(p.shape[0]), 1), float('nan'), dtype=torch.float64, device=p.device) for p in planes]
        else:
            planes = [np.full((p.shape[0], 1), np.nan) for p in planes]
    return hazard.site_hazard(*planes, groups, site_lon, site_lat, radius_km=radius_km, thresholds=thresholds,
                              return_max=return_max, engine=engine, device=device, n_groups=n_groups)


# ---------------------------------------------------------------------------------------------------------------- CLI
def _region(text):
    """NAME=LON0:LON1,LAT0:LAT1"""
    try:
        name, box = text.split('=', 1)
        lo, la = box.split(',')
        lon0, lon1 = (float(x) for x in lo.split(':'))
        lat0, lat1 = (float(x) for x in la.split(':'))
    except ValueError:
        raise argparse.ArgumentTypeError('--region: expected NAME=LON0:LON1,LAT0:LAT1, got %r' % text)
    if not name or not lat0 <= lat1 or not all(np.isfinite([lon0, lon1, lat0, lat1])):
        raise argparse.ArgumentTypeError('--region: need a name, finite bounds and LAT0 <= LAT1, got %r' % text)
    return name, (lon0, lon1, lat0, lat1)


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.landfall',
                                description='Landfall events, landfall intensity exceedance counts and return periods of track files.')
    p.add_argument('--land', required=True, metavar='land.nc', help="the model's land mask (intensity/data/land.nc schema)")
    analysis.add_site_args(p)
    p.add_argument('--region', type=_region, action='append', default=[], metavar='NAME=LON0:LON1,LAT0:LAT1',
                   help='repeatable; the box may cross the dateline (LON0 > LON1)')
    p.add_argument('--radius-km', type=float, default=100.0)
    analysis.add_threshold_arg(p)
    analysis.add_track_args(p, 'landfall.npz')
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    site_lon, site_lat = analysis.collect_sites(args)
    lon, lat, vmax, groups, gfile, gyear = analysis.load_groups(args.tracks)
    total_years = len(gfile)
    grid = read_land(args.land)
    ev = detect_landfalls(lon, lat, vmax, grid, device=args.device)
    c = landfall_counts(ev, groups, args.thresholds, regions=args.region, n_groups=total_years)
    out = dict(n_landfall=ev['n_landfall'], event_k=ev['k'], thresholds=c['thresholds'], groups=groups, total_years=total_years,
               **analysis.group_meta(args.tracks, gfile, gyear),
               counts_first=c['first'], counts_max=c['max'], n_storms=c['n_storms'],
               return_period_first=hazard.return_periods(c['first'][None], total_years)[0],
               return_period_max=hazard.return_periods(c['max'][None], total_years)[0],
               region_names=c['region_names'], region_box=c['region_box'], region_counts_first=c['region_first'],
               region_counts_max=c['region_max'], region_n_storms=c['region_n_storms'],
               region_return_period_first=hazard.return_periods(c['region_first'], total_years),
               region_return_period_max=hazard.return_periods(c['region_max'], total_years))
    for name in EVENT_FIELDS:
        out['event_' + name] = ev[name]
    if site_lon.size:
        r = landfall_site_hazard(ev, groups, site_lon, site_lat, radius_km=args.radius_km, thresholds=args.thresholds,
                                 device=args.device, n_groups=total_years)
        out.update(site_lon=site_lon, site_lat=site_lat, radius_km=args.radius_km, site_counts=r['counts'],
                   site_return_period=hazard.return_periods(r['counts'], total_years))
    np.savez(args.out, **out)
    n_lf = np.asarray(ev['n_landfall'])
    print('%d storms, %d make landfall (%d landfalls), %d groups (%d files), total_years = %d -> %s'
          % (lon.shape[0], int((n_lf > 0).sum()), int(n_lf.sum()), total_years, len(args.tracks), total_years, args.out))
    print('first-landfall return period (years) by threshold (m/s): ' + ' '.join('%6g' % t for t in c['thresholds']))
    print('  basin: ' + ' '.join('%6.3g' % v for v in out['return_period_first']))
    for i, name in enumerate(c['region_names']):
        print('  %s: ' % name + ' '.join('%6.3g' % v for v in out['region_return_period_first'][i]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
