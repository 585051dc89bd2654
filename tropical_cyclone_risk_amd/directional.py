"""Directional wind: the peak wind every storm of a track ensemble brings every site from each compass sector, how often each
sector brings at least given speeds, and the return periods per sector.

The wind is the footprint's (``windfield.py``): the same track, records, sub-steps, outer radius and per-pair wind, bit for bit.
On the GPU (``csrc/tcr_directional.hip``) the wind vector of every (site, record) pair is formed once:

1. its speed is the footprint's double, and ``theta`` is the direction it blows from, in degrees clockwise from north;
2. sector ``k`` of ``n_sector`` equal sectors holds the pairs with ``theta - sector0_deg`` in ``[(k - 1/2) W, (k + 1/2) W)`` mod
   360, ``W = 360 / n_sector``: with the defaults 0 is N, 1 NE, 2 E and so on.  A pair without wind has no sector;
3. per storm and sector, the peak over the sector's pairs within ``r_out_km`` of the site: NaN in every sector when the storm has
   no sample within ``r_out_km``, 0.0 in a sector no wind came from (the storm reached the site and did not exceed there);
4. per group of storms (a year, or an (ensemble file, year) pair) and sector, the number of storms whose peak is ``>=`` each of
   the ascending thresholds, and the return period ``total_years / exceedance_count``.

The maximum over the sectors is ``windfield.site_wind``'s ``site_max`` bit for bit.  The contract is the header's "directional
wind" section (include/tcrisk_hip.h).

    python -m tropical_cyclone_risk_amd.directional TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --out directional.npz

With ``--return-periods 10,50,100`` also the inverse, the wind of those return periods from every sector at every site (levels.py).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import analysis, hazard, windfield
from . import sitescan

MAX_SECTORS = 8
MAX_CELLS = sitescan.MAX_CELLS
# seven speeds: with the default eight sectors, 8 * (7 + 1) is the 64 cells a call may have
DEFAULT_THRESHOLDS = np.arange(10, 71, 10).astype(np.float64)
COMPASS = {1: ['all'], 4: ['N', 'E', 'S', 'W'], 8: ['N', 'NE', 'E', 'SE', 'S', 'SW', 'W', 'NW']}


def sector_centres(n_sector, sector0_deg=0.0):
    """[n_sector] the sectors' centre bearings (degrees clockwise from north, in [0, 360)): the direction the wind blows from."""
    return (float(sector0_deg) + np.arange(int(n_sector)) * (360.0 / int(n_sector))) % 360.0


def site_directional_wind(lon, lat, v, env, groups, site_lon, site_lat, dt_s, n_sector=8, sector0_deg=0.0,
                          thresholds=DEFAULT_THRESHOLDS, rmax_km=None, ck_cd=None, r_out_km=500., substeps=1, return_max=False,
                          engine=None, device=0, n_groups=None):
    """Peak footprint wind from each compass sector and its exceedance counts, at every site.

    lon, lat, v, env, dt_s, rmax_km, ck_cd, r_out_km, substeps, groups, n_groups, site_lon / site_lat, engine, device: as
    windfield.site_wind, under the same rules.  n_sector: 1 to 8 equal sectors.  sector0_deg: the centre bearing of sector 0,
    finite and in [0, 360).  thresholds: speeds (m/s), finite, strictly ascending; n_sector * (n_bin + 1) <= 64.  return_max:
    True, or a list of sector indices.  Returns a dict: ``counts`` [n_site][n_groups][n_sector][n_bin] int32, ``thresholds``,
    ``sector_from_deg`` [n_sector] (the sectors' centre bearings), and with ``return_max`` ``site_dir_max``
    [n_sector][n_site][n_trk] (m/s; NaN: no sample within r_out_km; 0.0: no wind from that sector; all NaN for a sector not asked
    for: a plane is n_site * n_trk * 8 bytes on the device, which is why they are selectable), in the type and on the device of
    ``lon``.
    """
    scan = _bind(groups, dt_s, n_sector, sector0_deg, thresholds, rmax_km, ck_cd, r_out_km, substeps, n_groups)
    res, fl = scan((lon, lat, v, env), site_lon, site_lat, return_max, engine, device)
    return sitescan.attach_planes(res, fl, 'site_dir_max', return_max, lon)


def _check_sectors(n_sector, sector0_deg, thresholds, return_max):
    """The analysis's own argument checks (ValueError): (n_sector, sector0_deg, the sorted sector indices whose planes are
    wanted)."""
    if isinstance(n_sector, bool) or int(n_sector) != n_sector or not 1 <= int(n_sector) <= MAX_SECTORS:
        raise ValueError('n_sector must be an integer in [1, %d]' % MAX_SECTORS)
    n_sector = int(n_sector)
    sector0_deg = float(sector0_deg)
    if not (np.isfinite(sector0_deg) and 0.0 <= sector0_deg < 360.0):
        raise ValueError('sector0_deg must be finite and in [0, 360)')
    thr = sitescan.check_ascending(thresholds, sitescan.ASCENDING % 'thresholds')
    if n_sector * (thr.size + 1) > MAX_CELLS:
        raise ValueError('n_sector * (n_bin + 1) must be <= %d' % MAX_CELLS)
    return n_sector, sector0_deg, sitescan.wanted_rows(return_max, n_sector, 'return_max', 'sector')


def _bind(groups, dt_s, n_sector, sector0_deg, thresholds, rmax_km, ck_cd, r_out_km, substeps, n_groups):
    """site_directional_wind's arguments, checked as far as they stand alone (_check_sectors) and bound into sitescan's
    scan(tracks = (lon, lat, v, env), site_lon, site_lat, want, engine, device): one call of tcr_directional_*, whose ``planes`` are
    those of the sectors in want (a return_max).  windfield._prepare needs the tracks: it runs in every call, after want's check."""
    n_sector, sector0_deg, _ = _check_sectors(n_sector, sector0_deg, thresholds, False)

    def scan(tracks, site_lon, site_lat, want=(), engine=None, device=0):
        want = sitescan.wanted_rows(want, n_sector, 'return_max', 'sector')
        planes, fl, thr, prm = windfield._prepare(tracks, dt_s, rmax_km, ck_cd, r_out_km, substeps, thresholds, n_groups)

        def make_args(a, rows):
            n_bin_, thr_, counts_, _ = a.out
            return (C.byref(windfield._tracks_struct(a)), C.byref(prm)) + a.sites + (n_sector, sector0_deg, n_bin_, thr_, counts_, rows)
        res = sitescan.stacked_scan('tcr_directional', planes, fl, groups, n_groups, site_lon, site_lat, thr, n_sector, want, 'dir',
                                    engine, device, make_args)
        res['sector_from_deg'] = sector_centres(n_sector, sector0_deg)
        return res, fl
    return scan


def return_periods(counts, total_years):
    """[n_site][n_sector][n_bin] total_years / exceedance count of counts [n_site][n_groups][n_sector][n_bin], summed over the
    groups (hazard.return_periods: ``inf`` where the count is 0)."""
    c = analysis.to_numpy(counts).sum(axis=1)
    return hazard.return_periods(c.reshape(c.shape[0], -1), total_years).reshape(c.shape)


def worst_sector(counts, total_years):
    """Per site (sector, threshold index, return period) of the sector with the shortest return period at the highest threshold
    any sector reaches; (-1, -1, inf) for a site no threshold is reached at."""
    c = analysis.to_numpy(counts).sum(axis=1)
    out = []
    for ci in c:
        reached = np.nonzero(ci.any(axis=0))[0]
        if reached.size == 0:
            out.append((-1, -1, np.inf))
            continue
        b = int(reached[-1])
        k = int(np.argmax(ci[:, b]))
        out.append((k, b, float(total_years) / float(ci[k, b])))
    return out


# ---------------------------------------------------------------------------------------------------------------- CLI
def _parse_thresholds(text):
    """LO:HI:STEP, or V1,V2,..."""
    if ':' in text:
        return analysis.parse_range(text, '--thresholds')
    try:
        return np.array([float(x) for x in text.split(',')])
    except ValueError:
        raise argparse.ArgumentTypeError('--thresholds: expected LO:HI:STEP or V1,V2,..., got %r' % text)


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.directional',
                                description='Peak footprint wind by the compass sector it blows from, at sites: exceedance counts '
                                            'and return periods per sector.')
    analysis.add_site_args(p)
    analysis.add_footprint_args(p)
    p.add_argument('--sectors', type=int, default=8, metavar='N', help='1 to 8 equal compass sectors (default 8: N, NE, E, ...)')
    p.add_argument('--sector0-deg', type=float, default=0.0, metavar='DEG',
                   help='centre bearing of sector 0, degrees clockwise from north in [0, 360) (default 0)')
    p.add_argument('--thresholds', type=_parse_thresholds, default=DEFAULT_THRESHOLDS, metavar='LO:HI:STEP',
                   help='speeds in m/s; sectors * (thresholds + 1) <= 64 (default: %s)' % ' '.join('%g' % t for t in DEFAULT_THRESHOLDS))
    analysis.add_return_period_arg(p, 'peak wind (m/s) from every sector')
    analysis.add_track_args(p, 'directional.npz')
    a = analysis.finish_parse(p, p.parse_args(argv), no_tail='--tail-exceedances is not offered for directional wind: a sector\'s '
                              'peaks have a point mass at 0 (storms that reached the site with no wind from that sector), which a '
                              'Pareto fit to the excesses does not describe')
    try:
        _check_sectors(a.sectors, a.sector0_deg, a.thresholds, False)
    except ValueError as e:
        p.error(str(e))
    return a


def _sector_name(k, n_sector, centres):
    names = COMPASS.get(n_sector)
    return '%d (from %g deg%s)' % (k, centres[k], ', ' + names[k] if names and centres[0] == 0.0 else '')


def main(argv=None):
    args = parse_args(argv)
    inp = analysis.load_inputs(args, wind=True)
    site_lon, site_lat, total_years = inp.site_lon, inp.site_lat, inp.total_years
    tracks = (inp.lon, inp.lat, inp.v, tuple(inp.env))
    scan = _bind(inp.groups, inp.dt_s, args.sectors, args.sector0_deg, args.thresholds, args.rmax_km, args.ck_cd, args.r_out_km,
                 args.substeps, total_years)
    res, _ = scan(tracks, site_lon, site_lat, device=args.device)
    more = {}
    if args.return_periods is not None:
        more = sitescan.stacked_return_levels(scan, args.sectors, tracks, site_lon, site_lat, total_years, args.return_periods,
                                              args.device)
    rp = return_periods(res['counts'], total_years)
    centres, thr = res['sector_from_deg'], res['thresholds']
    analysis.save_npz(args, inp, dict(counts=res['counts'], return_period=rp, sector_from_deg=centres, thresholds=thr),
                      recorded=('r_out_km', 'substeps', 'rmax_km'), more=more)
    analysis.print_summary(args, inp, ', r_out = %g km, %d substeps, %d sectors' % (args.r_out_km, args.substeps, args.sectors))
    if site_lon.size <= 10:
        worst = ['no sector reaches %g m/s' % thr[0] if k < 0 else
                 'worst sector %s: %g m/s every %.3g years' % (_sector_name(k, args.sectors, centres), thr[b], period)
                 for k, b, period in worst_sector(res['counts'], total_years)]
        analysis.print_site_rows(None, site_lon, site_lat, worst)
        for k in range(args.sectors if more else 0):
            analysis.print_site_rows('peak wind (m/s) from sector %s by return period (years): ' % _sector_name(k, args.sectors, centres)
                                     + ' '.join('%6g' % t for t in more['return_periods']), site_lon, site_lat,
                                     more['return_level'][:, k], '%6.4g')
    return 0


if __name__ == '__main__':
    sys.exit(main())
