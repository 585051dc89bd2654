"""Wind duration: for how long every storm of a track ensemble brings every site a wind of at least each of a few levels, how
often it does so for at least so many hours, and the expected hours per year.

The wind is the footprint's (``windfield.py``): the same track, records, sub-steps, outer radius and per-pair wind, bit for bit.
On the GPU (``csrc/tcr_duration.hip``) it is evaluated once per (site, record) pair and compared with all levels at once:

1. record ``q`` of a storm carries the integer half-weight 2, or 1 at the two ends of the track (the trapezoid rule in units of
   half a sub-step); ``H`` is the sum of the half-weights of the records within ``r_out_km`` of the site whose wind is ``>=`` the
   level, and the storm's hours there are ``H * hours_per_half_step`` with ``hours_per_half_step = dt_s / (7200 substeps)``
   (NaN when no record is within ``r_out_km``, 0 when none reaches the level);
2. per group of storms (a year, or an (ensemble file, year) pair) and level, the number of storms whose hours are ``>=`` each of
   the ascending duration thresholds, and the sum of ``H`` (``half_steps``): the hours per year at or above a level are
   ``half_steps.sum(groups) * hours_per_half_step / total_years``;
3. the return period ``total_years / exceedance_count`` (``hazard.return_periods``).

Everything accumulated is an integer, so every output is bit-identical whatever the site order, the storm order and the launch
shape.  The contract is the header's "wind duration" section (include/tcrisk_hip.h).  Not modelled: duration is quantised to
``dt_s / (2 substeps)``, and a crossing of a level between two records is not interpolated.

    python -m tropical_cyclone_risk_amd.duration TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --out duration.npz

With ``--return-periods 10,50,100`` also the inverse, the hours of those return periods at every site and level (levels.py).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis, hazard, windfield
from . import sitescan

MAX_LEVELS = 8
MAX_CELLS = sitescan.MAX_CELLS
DEFAULT_LEVELS = np.array([34.0, 50.0, 64.0]) * 1852.0 / 3600.0          # gale, storm and hurricane force (kt) in m/s
DEFAULT_HOURS = np.array([1, 3, 6, 12, 24, 48], dtype=np.float64)


def hours_per_half_step(dt_s, substeps):
    """u of the contract: the hours one half-weight stands for."""
    return float(dt_s) / (7200.0 * int(substeps))


def site_duration(lon, lat, v, env, groups, site_lon, site_lat, dt_s, levels=DEFAULT_LEVELS, thresholds=DEFAULT_HOURS, rmax_km=None,
                  ck_cd=None, r_out_km=500., substeps=1, return_hours=False, engine=None, device=0, n_groups=None):
    """Hours at or above wind levels, their exceedance counts and their totals, at every site.

    lon, lat, v, env, dt_s, rmax_km, ck_cd, r_out_km, substeps, groups, n_groups, site_lon / site_lat, engine, device: as
    windfield.site_wind, under the same rules.  levels: 1 to 8 wind levels (m/s), finite, > 0, strictly ascending.  thresholds:
    durations (hours), finite, > 0, strictly ascending; n_level * (n_bin + 1) <= 64.  return_hours: True, or a list of level
    indices.  Returns a dict: ``counts`` [n_site][n_groups][n_level][n_bin] int32, ``half_steps`` [n_site][n_groups][n_level]
    int64, ``hours_per_half_step``, ``levels``, ``thresholds``, and with ``return_hours`` ``site_hours``
    [n_level][n_site][n_trk] (hours; NaN: no sample within r_out_km; all NaN for a level not asked for: a plane is
    n_site * n_trk * 8 bytes on the device, which is why they are selectable), in the type and on the device of ``lon``.
    """
    scan = _bind(groups, dt_s, levels, thresholds, rmax_km, ck_cd, r_out_km, substeps, n_groups)
    res, fl = scan((lon, lat, v, env), site_lon, site_lat, return_hours, engine, device)
    return sitescan.attach_planes(res, fl, 'site_hours', return_hours, lon)


def _check_levels(levels, thresholds, return_hours):
    """The duration's own argument checks (ValueError): (levels, the sorted level indices whose planes are wanted)."""
    lev = np.ascontiguousarray(np.asarray(levels, dtype=np.float64).reshape(-1))
    if not 1 <= lev.size <= MAX_LEVELS:
        raise ValueError('give 1 to %d levels' % MAX_LEVELS)
    lev = sitescan.check_ascending(lev, sitescan.ASCENDING_POSITIVE % 'levels', positive=True)
    thr = sitescan.check_ascending(thresholds, sitescan.ASCENDING_POSITIVE % 'thresholds', positive=True)
    if lev.size * (thr.size + 1) > MAX_CELLS:
        raise ValueError('n_level * (n_bin + 1) must be <= %d' % MAX_CELLS)
    return lev, sitescan.wanted_rows(return_hours, lev.size, 'return_hours', 'level')


def _bind(groups, dt_s, levels, thresholds, rmax_km, ck_cd, r_out_km, substeps, n_groups):
    """site_duration's arguments, checked as far as they stand alone (_check_levels) and bound into sitescan's
    scan(tracks = (lon, lat, v, env), site_lon, site_lat, want, engine, device): one call of tcr_duration_*, whose ``planes`` are
    those of the levels in want (a return_hours).  windfield._prepare needs the tracks: it runs in every call, after want's check."""
    lev, _ = _check_levels(levels, thresholds, False)
    n_level = int(lev.size)

    def scan(tracks, site_lon, site_lat, want=(), engine=None, device=0):
        want = sitescan.wanted_rows(want, n_level, 'return_hours', 'level')
        planes, fl, thr, prm = windfield._prepare(tracks, dt_s, rmax_km, ck_cd, r_out_km, substeps, thresholds, n_groups)

        def make_args(a, hours):
            n_bin_, thr_, counts_, _ = a.out
            return (C.byref(windfield._tracks_struct(a)), C.byref(prm)) + a.sites + \
                (n_level, lev.ctypes.data_as(_lib.DP), n_bin_, thr_, counts_, a.outputs[0], hours)
        res = sitescan.stacked_scan('tcr_duration', planes, fl, groups, n_groups, site_lon, site_lat, thr, n_level, want, 'hours',
                                    engine, device, make_args, more_outputs=[('half_steps', ('site_group', n_level))])
        res['hours_per_half_step'] = hours_per_half_step(prm.dt_s, prm.substeps)
        res['levels'] = lev
        return res, fl
    return scan


# ---------------------------------------------------------------------------------------------------------------- CLI
def _parse_levels(text):
    try:
        lev = np.array([float(x) for x in text.split(',')])
    except ValueError:
        raise argparse.ArgumentTypeError('--levels: expected L1,L2,... (m/s), got %r' % text)
    return lev


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.duration',
                                description='Hours at or above wind levels at sites: exceedance counts of durations, their return '
                                            'periods and the expected hours per year.')
    analysis.add_site_args(p)
    analysis.add_footprint_args(p)
    p.add_argument('--levels', type=_parse_levels, default=DEFAULT_LEVELS, metavar='L1,L2,...',
                   help='1 to 8 ascending wind levels in m/s (default: 34, 50 and 64 kt)')
    p.add_argument('--thresholds', type=lambda t: analysis.parse_range(t, '--thresholds'), default=DEFAULT_HOURS, metavar='LO:HI:STEP',
                   help='durations in hours (default: %s)' % ' '.join('%g' % t for t in DEFAULT_HOURS))
    analysis.add_return_period_arg(p, 'hours at or above every level')
    analysis.add_track_args(p, 'duration.npz')
    a = analysis.finish_parse(p, p.parse_args(argv), no_tail='--tail-exceedances is not offered for durations: they are quantised in '
                              'half sub-steps, which a Pareto fit to the excesses does not describe')
    try:
        _check_levels(a.levels, a.thresholds, False)
    except ValueError as e:
        p.error(str(e))
    return a


def main(argv=None):
    args = parse_args(argv)
    inp = analysis.load_inputs(args, wind=True)
    site_lon, site_lat, total_years = inp.site_lon, inp.site_lat, inp.total_years
    tracks = (inp.lon, inp.lat, inp.v, tuple(inp.env))
    scan = _bind(inp.groups, inp.dt_s, args.levels, args.thresholds, args.rmax_km, args.ck_cd, args.r_out_km, args.substeps, total_years)
    res, _ = scan(tracks, site_lon, site_lat, device=args.device)
    lev = res['levels']
    annual = res['half_steps'].sum(axis=1) * res['hours_per_half_step'] / total_years
    more = {}
    if args.return_periods is not None:
        more = sitescan.stacked_return_levels(scan, lev.size, tracks, site_lon, site_lat, total_years, args.return_periods, args.device)
    rp = hazard.return_periods(res['counts'], total_years)
    analysis.save_npz(args, inp, dict(counts=res['counts'], return_period=rp, annual_hours=annual, levels=lev,
                                      thresholds=res['thresholds']), more=more)
    analysis.print_summary(args, inp, ', r_out = %g km, %d substeps' % (args.r_out_km, args.substeps))
    if site_lon.size <= 10:
        analysis.print_site_rows('hours per year at or above (m/s): ' + ' '.join('%8.4g' % x for x in lev), site_lon, site_lat,
                                 annual, '%8.4g')
        for l, x in enumerate(lev if more else ()):
            analysis.print_site_rows('hours at or above %.4g m/s by return period (years): ' % x
                                     + ' '.join('%6g' % t for t in more['return_periods']), site_lon, site_lat,
                                     more['return_level'][:, l], '%6.4g')
    return 0


if __name__ == '__main__':
    sys.exit(main())
