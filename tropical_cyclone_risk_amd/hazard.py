"""Site wind hazard: near-site intensity, exceedance counts and return periods of a track ensemble.

The analysis of the reference's ``notebooks/sample_analysis.ipynb``, for many sites at once and on the GPU
(``csrc/tcr_hazard.hip``):

1. for each storm, the maximum ``vmax_trks`` over its samples within ``radius_km`` (the notebook's haversine,
   r_earth = 6378 km) of a site (NaN when there are none);
2. per group of storms (a year, or an (ensemble file, year) pair), the number of storms whose value is ``>= v`` for
   ascending thresholds ``v``;
3. the return period ``total_years / exceedance_count`` (``inf`` where the count is 0).

    python -m tropical_cyclone_risk_amd.hazard TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --out hazard.npz
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib
from .basins import BASIN_IDS

DEFAULT_THRESHOLDS = np.arange(10, 81, 5).astype(np.float64)


def _is_tensor(x):
    return type(x).__module__.startswith('torch')


def _spatial_order(lon, lat, xp):
    """Z-order (Morton) of the sites on a 2^16 x 2^16 lon / lat raster: runs of consecutive sites are compact patches, which
    is what the kernel's per-64-site culling wants.  `xp` is numpy or torch (the same integer operations on both)."""
    to_int = (lambda a: a.astype(np.int64)) if xp is np else (lambda a: a.long())
    qx = to_int((lon % 360.0) * (65535.0 / 360.0))
    qy = to_int((lat + 90.0).clip(0.0, 180.0) * (65535.0 / 180.0))

    def spread(v):
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555
    key = spread(qx) | (spread(qy) << 1)
    return xp.argsort(key, stable=True) if xp is not np else np.argsort(key, kind='stable')


class _Context:
    """The caller's engine (anything with a library handle `.h`), or a context of our own for one call."""

    def __init__(self, engine, device):
        self.L = _lib.lib()
        self.own = engine is None
        if self.own:
            h = C.c_void_p()
            if self.L.tcr_ctx_create(int(device), C.byref(h)) != 0:
                raise _lib.TcrError(self.L.tcr_last_error(None).decode())
            self.h = h
        else:
            self.h = engine.h

    def check(self, rc):
        if rc != 0:
            raise _lib.TcrError(self.L.tcr_last_error(self.h).decode())

    def close(self):
        if self.own and self.h:
            self.L.tcr_ctx_destroy(self.h)
            self.h = None


def _as_planes(arrays, names):
    """The track planes as fp64 arrays of the type and on the device of the first: (planes, conv), conv being the conversion."""
    first = arrays[0]
    if _is_tensor(first):
        import torch
        conv = lambda a: torch.as_tensor(a, dtype=torch.float64, device=first.device)     # noqa: E731
    else:
        conv = lambda a: np.asarray(a.cpu() if _is_tensor(a) else a, dtype=np.float64)    # noqa: E731
    planes = [conv(a) for a in arrays]
    if planes[0].ndim != 2 or any(tuple(p.shape) != tuple(planes[0].shape) for p in planes):
        raise ValueError('%s must be [n_trk][n_t] arrays of one shape' % names)
    return planes, conv


def _site_scan(entry, planes, conv, groups, n_groups, site_lon, site_lat, thr, return_max, engine, device, make_args,
               site_extras=(), more_outputs=()):
    """What the per-site analyses (csrc/tcr_sitescan.h) share in front of the library: checks the sites and groups, puts the
    storms of a group next to each other and the sites in spatial order, runs ``entry + '_dev'`` (torch tensors, on the current
    stream) or ``entry + '_host'`` (NumPy) and returns ``counts``, ``thresholds`` and with return_max ``site_max`` in the
    caller's site and storm order.  planes, conv: of _as_planes.  make_args(tracks, sites, out) -> the entry point's arguments
    after the context: tracks holds the fields every tracks struct has and ``planes``, the pointers of the permuted planes;
    sites = (n_site, lon, lat) and out = (n_bin, thresholds, counts, site_max) are ready to pass on.  The library is not
    touched before every check here has passed.

    An analysis with more per-site inputs or more outputs (loss.py) names them: site_extras, [n_site] arrays (or None) that go
    through the site permutation with the coordinates; more_outputs, (name, axis) pairs of fp64 outputs along 'trk', 'group' or
    'site', which come back under their names in the caller's order.  make_args then gets a fourth argument,
    (pointers of the extras (None stays None), pointers of the outputs)."""
    torch_in = _is_tensor(planes[0])
    if torch_in:
        import torch
        xp = torch
        dev = planes[0].device
        device = dev.index if dev.index is not None else torch.cuda.current_device()
    else:
        xp = np
    site_lon, site_lat = (conv(a).reshape(-1) for a in (site_lon, site_lat))
    if site_lon.shape[0] != site_lat.shape[0] or site_lon.shape[0] < 1:
        raise ValueError('site_lon and site_lat must be non-empty and of one length')
    if not bool(xp.isfinite(site_lon).all()) or not bool(xp.isfinite(site_lat).all()):
        raise ValueError('site coordinates must be finite')
    site_extras = [None if a is None else conv(a).reshape(-1) for a in site_extras]
    if any(a is not None and a.shape[0] != site_lon.shape[0] for a in site_extras):
        raise ValueError('a per-site array must hold one value per site')
    n_trk, n_t = int(planes[0].shape[0]), int(planes[0].shape[1])
    g = np.asarray(groups.cpu() if _is_tensor(groups) else groups).reshape(-1)
    if g.shape[0] != n_trk or (n_trk and (g.dtype.kind not in 'iu' or g.min() < 0)):
        raise ValueError('groups must hold one non-negative integer per storm')
    g = g.astype(np.int64)
    n_groups = int(n_groups if n_groups is not None else (g.max() + 1 if n_trk else 1))
    if n_trk and g.max() >= n_groups:
        raise ValueError('a group index is >= n_groups')

    # storms grouped contiguously (stable: storms keep their order inside a group), sites in spatial order
    order = np.argsort(g, kind='stable')
    group_off = np.zeros(n_groups + 1, dtype=np.int64)
    group_off[1:] = np.cumsum(np.bincount(g, minlength=n_groups))
    sorted_ = bool(np.all(order == np.arange(n_trk)))
    site_order = _spatial_order(site_lon, site_lat, xp)
    n_site, n_bin = int(site_lon.shape[0]), int(thr.shape[0])
    if torch_in:
        idx = torch.as_tensor(order, device=dev)
        planes = [(a if sorted_ else a.index_select(0, idx)).contiguous() for a in planes]
        slon, slat = site_lon[site_order].contiguous(), site_lat[site_order].contiguous()
        counts = torch.empty((n_site, n_groups, max(n_bin, 1)), dtype=torch.int32, device=dev)
        smax = torch.empty((n_site, max(n_trk, 1)), dtype=torch.float64, device=dev) if return_max else None
        extras = [None if a is None else a[site_order].contiguous() for a in site_extras]
        new = lambda n: torch.empty(max(n, 1), dtype=torch.float64, device=dev)           # noqa: E731
    else:
        planes = [np.ascontiguousarray(a if sorted_ else a[order]) for a in planes]
        slon, slat = np.ascontiguousarray(site_lon[site_order]), np.ascontiguousarray(site_lat[site_order])
        counts = np.empty((n_site, n_groups, max(n_bin, 1)), dtype=np.int32)
        smax = np.empty((n_site, max(n_trk, 1)), dtype=np.float64) if return_max else None
        extras = [None if a is None else np.ascontiguousarray(a[site_order]) for a in site_extras]
        new = lambda n: np.empty(max(n, 1), dtype=np.float64)                             # noqa: E731
    more = [new(dict(trk=n_trk, group=n_groups, site=n_site)[axis]) for _, axis in more_outputs]
    ptr = (lambda a: a.data_ptr()) if torch_in else (lambda a: a.ctypes.data)
    tracks = dict(n_trk=n_trk, n_t=n_t, row_stride=n_t, n_group=n_groups, group_off=group_off.ctypes.data_as(C.POINTER(C.c_int64)),
                  planes=[ptr(a) for a in planes])
    args = (tracks, (n_site, ptr(slon), ptr(slat)),
            (n_bin, thr.ctypes.data_as(_lib.DP), ptr(counts), ptr(smax) if smax is not None else None))
    if site_extras or more_outputs:
        args += (([None if a is None else ptr(a) for a in extras], [ptr(a) for a in more]),)
    args = make_args(*args)
    ctx = _Context(engine, device)
    try:
        if torch_in:
            ctx.check(getattr(ctx.L, entry + '_dev')(ctx.h, *args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        else:
            ctx.check(getattr(ctx.L, entry + '_host')(ctx.h, *args))
    finally:
        if torch_in and ctx.own:
            torch.cuda.current_stream(dev).synchronize()       # the context's workspaces go with it
        ctx.close()

    # back to the caller's site and storm order
    out_counts = xp.empty_like(counts)
    out_counts[site_order] = counts
    res = dict(counts=out_counts, thresholds=thr)
    for (name, axis), a in zip(more_outputs, more):
        if axis == 'group':
            res[name] = a[:n_groups]
            continue
        out = xp.empty_like(a[:n_trk] if axis == 'trk' else a)
        if axis == 'site':
            out[site_order] = a
        else:
            out[idx if torch_in else order] = a[:n_trk]
        res[name] = out
    if return_max and torch_in:
        m = smax[:, :n_trk]
        out = torch.empty_like(m)
        out[site_order] = m
        if not sorted_:
            un = torch.empty_like(out)
            un[:, idx] = out
            out = un
        res['site_max'] = out
    elif return_max:
        out = np.empty((n_site, n_trk))
        out[np.ix_(site_order, order)] = smax[:, :n_trk]
        res['site_max'] = out
    return res


def site_hazard(lon, lat, vmax, groups, site_lon, site_lat, radius_km=100., thresholds=DEFAULT_THRESHOLDS, return_max=False,
                engine=None, device=0, n_groups=None):
    """Near-site intensity and exceedance counts of every site.

    lon, lat, vmax: [n_trk][n_t] fp64 (the track file's lon_trks, lat_trks, vmax_trks; NaN past a track's end), NumPy arrays or
    torch tensors on the GPU (then everything stays there).  groups: [n_trk] integer group of every storm, in [0, n_groups)
    (default n_groups = max + 1; a group without storms counts 0).  site_lon / site_lat: [n_site], either longitude convention.
    Returns a dict: ``counts`` [n_site][n_groups][n_bin] int32 (storms of the group whose near-site maximum is >= the threshold),
    ``thresholds``, and with ``return_max`` ``site_max`` [n_site][n_trk] (NaN: no sample within the radius).  Arrays come back
    in the type and on the device of ``lon``.  ``engine``: a TCEngine whose context is used (None: one is opened for the call).
    The library checks ``radius_km`` and ``thresholds`` (``_lib.TcrError``).
    """
    planes, conv = _as_planes((lon, lat, vmax), 'lon, lat and vmax')
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))

    def make_args(tracks, sites, out):
        lon_, lat_, vmax_ = tracks.pop('planes')
        return (C.byref(_lib.HazardTracks(lon=lon_, lat=lat_, vmax=vmax_, **tracks)),) + sites + (float(radius_km),) + out
    return _site_scan('tcr_hazard', planes, conv, groups, n_groups, site_lon, site_lat, thr, return_max, engine, device, make_args)


def return_periods(counts, total_years):
    """total_years / exceedance count (the notebook's formula), ``inf`` where the count is 0.  counts: [..][n_group][n_bin]
    (summed over groups) or [n_site][n_bin] already summed (2-D)."""
    c = np.asarray(counts.cpu() if _is_tensor(counts) else counts)
    if c.ndim == 3:
        c = c.sum(axis=1)
    c = c.astype(np.float64)
    with np.errstate(divide='ignore'):
        return np.where(c > 0, float(total_years) / np.where(c > 0, c, 1.0), np.inf)


def storm_frequency(seeds_per_month, basin_id, tracks_per_year, obs_tracks_per_year):
    """The notebook's seed-survival calibration of the interannual storm frequency.

    seeds_per_month: [ensemble][year][basin][month] (or one file's [year][basin][month]) seeds a file needed per month; the
    seeds are summed over ensemble files and months, gamma = tracks_per_year / seeds, c = obs_tracks_per_year / mean(gamma),
    and the frequency is c * gamma, one value per year."""
    s = np.asarray(seeds_per_month, dtype=np.float64)
    if s.ndim == 3:
        s = s[None]
    if s.ndim != 4 or s.shape[2] != len(BASIN_IDS):
        raise ValueError('seeds_per_month must be [ensemble][year][basin][month] with %d basins' % len(BASIN_IDS))
    total = s[:, :, BASIN_IDS.index(basin_id), :].sum(axis=(0, 2))
    gamma = tracks_per_year / total
    return (obs_tracks_per_year / gamma.mean()) * gamma


# ---------------------------------------------------------------------------------------------------------------- CLI
def _range(text, what):
    """LO:HI:STEP, both ends included."""
    try:
        lo, hi, step = (float(x) for x in text.split(':'))
    except ValueError:
        raise argparse.ArgumentTypeError('%s: expected LO:HI:STEP, got %r' % (what, text))
    if not step > 0 or hi < lo:
        raise argparse.ArgumentTypeError('%s: need STEP > 0 and HI >= LO, got %r' % (what, text))
    return lo + step * np.arange(int(np.floor((hi - lo) / step + 1e-9)) + 1)


def _site(text):
    try:
        lon, lat = (float(x) for x in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('--site: expected LON,LAT, got %r' % text)
    return lon, lat


def _grid(text):
    parts = text.split(',')
    if len(parts) != 2:
        raise argparse.ArgumentTypeError('--grid: expected LON0:LON1:DLON,LAT0:LAT1:DLAT, got %r' % text)
    return _range(parts[0], '--grid lon'), _range(parts[1], '--grid lat')


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.hazard',
                                description='Near-site intensity exceedance counts and return periods of track files.')
    p.add_argument('tracks', nargs='+', help='track files (ensemble members); every year of every file is one group')
    p.add_argument('--site', type=_site, action='append', default=[], metavar='LON,LAT',
                   help='repeatable; write --site=LON,LAT when LON is negative')
    p.add_argument('--sites', metavar='FILE.csv', help='one LON,LAT per line (lines that are not two numbers are skipped)')
    p.add_argument('--grid', type=_grid, metavar='LON0:LON1:DLON,LAT0:LAT1:DLAT')
    p.add_argument('--radius-km', type=float, default=100.0)
    p.add_argument('--thresholds', type=lambda t: _range(t, '--thresholds'), default=DEFAULT_THRESHOLDS, metavar='LO:HI:STEP')
    p.add_argument('--out', default='hazard.npz')
    p.add_argument('--device', type=int, default=0)
    a = p.parse_args(argv)
    if not (a.site or a.sites or a.grid):
        p.error('give sites with --site, --sites or --grid')
    return a


def read_sites_csv(fn):
    out = []
    for line in open(fn):
        f = line.replace(';', ',').split(',')
        try:
            if len(f) >= 2:
                out.append((float(f[0]), float(f[1])))
        except ValueError:
            pass
    return out


def collect_sites(args):
    """The sites of --site, --sites and --grid, in that order: (lon [n], lat [n])."""
    pts = list(args.site)
    if args.sites:
        pts += read_sites_csv(args.sites)
    lon = [p[0] for p in pts]
    lat = [p[1] for p in pts]
    if args.grid is not None:
        glon, glat = np.meshgrid(args.grid[0], args.grid[1])
        lon += list(glon.ravel())
        lat += list(glat.ravel())
    return np.array(lon, dtype=np.float64), np.array(lat, dtype=np.float64)


def load_groups(files, extra=()):
    """Read the track files and number their (file, year) groups: every year of every file's `year` coordinate is one group,
    years without storms included.  Returns lon, lat, vmax [n_trk][n_t], the group of every storm, group_file and group_year
    [n_group] (the group -> (file index, year) map).  extra: names of further variables of the files; when given, a seventh
    element {name: [one array per file]} follows."""
    from . import io as tio
    lon, lat, vmax, groups, gfile, gyear = [], [], [], [], [], []
    more = {name: [] for name in extra}
    for k, fn in enumerate(files):
        d = tio.read_tracks(fn)
        for name in extra:
            more[name].append(np.asarray(d[name]))
        years = np.asarray(d['year']).astype(np.int64).reshape(-1)
        tc_years = np.asarray(d['tc_years']).astype(np.int64).reshape(-1)
        pos = {int(y): i for i, y in enumerate(years)}
        if not set(int(y) for y in tc_years) <= set(pos):
            raise ValueError('%s: a storm year is not in the file\'s year coordinate' % fn)
        groups.append(len(gfile) + np.array([pos[int(y)] for y in tc_years], dtype=np.int64))
        gfile += [k] * len(years)
        gyear += list(years)
        for dst, key in ((lon, 'lon_trks'), (lat, 'lat_trks'), (vmax, 'vmax_trks')):
            dst.append(np.asarray(d[key], dtype=np.float64))
    n_t = {a.shape[1] for a in lon}
    if len(n_t) != 1:
        raise ValueError('the track files have different time axes: %s' % sorted(n_t))
    res = (np.concatenate(lon), np.concatenate(lat), np.concatenate(vmax), np.concatenate(groups),
           np.array(gfile, dtype=np.int64), np.array(gyear, dtype=np.int64))
    return res + (more,) if extra else res


def main(argv=None):
    args = parse_args(argv)
    site_lon, site_lat = collect_sites(args)
    if site_lon.size == 0:
        raise SystemExit('no sites')
    lon, lat, vmax, groups, gfile, gyear = load_groups(args.tracks)
    total_years = len(gfile)
    res = site_hazard(lon, lat, vmax, groups, site_lon, site_lat, radius_km=args.radius_km, thresholds=args.thresholds,
                      device=args.device, n_groups=total_years)
    rp = return_periods(res['counts'], total_years)
    np.savez(args.out, counts=res['counts'], return_period=rp, thresholds=res['thresholds'], site_lon=site_lon, site_lat=site_lat,
             total_years=total_years, radius_km=args.radius_km, group_file=gfile, group_year=gyear,
             files=np.array([str(f) for f in args.tracks]))
    print('%d sites, %d storms, %d groups (%d files), total_years = %d -> %s'
          % (site_lon.size, lon.shape[0], total_years, len(args.tracks), total_years, args.out))
    if site_lon.size <= 10:
        print('return period (years) by threshold (m/s): ' + ' '.join('%6g' % t for t in res['thresholds']))
        for i in range(site_lon.size):
            print('  site (%.4f, %.4f): ' % (site_lon[i], site_lat[i]) + ' '.join('%6.3g' % v for v in rp[i]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
