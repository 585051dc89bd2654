"""Compound wind-rain hazard: how often a site gets a footprint wind of at least ``u`` and a storm rain of at least ``p`` from the
same storm, how often it gets either, and the return periods of both.

The wind is the footprint's (``windfield.py``), the rain the rainfall's (``rainfall.py``), each with its own outer radius, on the
track the two share: a storm's leading run of samples where all eight planes are finite.  On the GPU
(``csrc/tcr_compound.hip``) both are evaluated in one scan of the ensemble, which shares the culling, the distance test and the
angle of every (site, record) pair between them, and the joint histogram is built there: the two [n_site][n_trk] planes a joint
count would otherwise need are optional outputs.

``counts[site][group][a][b]`` is the number of storms of the group that pass at least ``a`` wind thresholds and at least ``b`` rain
thresholds.  Index 0 on an axis means "no condition on this hazard": ``counts[..., 1:, 0]`` are the wind footprint's counts,
``counts[..., 0, 1:]`` the rainfall's, ``counts[..., 1:, 1:]`` the joint (AND) table, ``counts[..., 0, 0]`` the group's size;
``or_counts`` gives the OR table by inclusion-exclusion.

The contract is the header's "compound hazard" section (include/tcrisk_hip.h).

    python -m tropical_cyclone_risk_amd.compound TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --out compound.npz
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis, hazard, rainfall, windfield
from .sitescan import MAX_CELLS, site_scan          # MAX_CELLS bounds (n_wbin + 1) * (n_rbin + 1)

DEFAULT_WIND_THRESHOLDS = np.arange(20, 71, 10).astype(np.float64)                     # m/s
DEFAULT_RAIN_THRESHOLDS = np.arange(50, 401, 50).astype(np.float64)                    # mm
RAIN_KEY = {'total': 'site_rain', 'peak-rate': 'site_peak_rate'}


def site_compound(lon, lat, v, vmax, env, groups, site_lon, site_lat, dt_s, wind_thresholds, rain_thresholds, rmax_km=None,
                  ck_cd=None, wind_r_out_km=500., rain_r_out_km=500., substeps=1, stat='total', coefficients=None, v_lo_kt=35.,
                  v_hi_kt=155., return_values=False, engine=None, device=0, n_groups=None):
    """Joint exceedance counts of footprint wind and storm rain of every site.

    lon, lat, v, env, rmax_km, ck_cd: as windfield.site_wind; vmax, stat, coefficients, v_lo_kt, v_hi_kt: as rainfall.site_rain.
    A storm's track is its leading run of samples where all eight planes are finite.  wind_r_out_km, rain_r_out_km: each
    hazard's own outer radius; dt_s and substeps are common to both.  wind_thresholds (m/s), rain_thresholds (mm, or mm/h for
    'peak-rate'): finite, strictly ascending, with (n_wbin + 1) * (n_rbin + 1) <= 64.  groups, n_groups, site_lon / site_lat,
    engine, device: as hazard.site_hazard.  NumPy arrays or torch tensors on the GPU (then everything stays there).  Returns a
    dict: ``counts`` [n_site][n_groups][n_wbin + 1][n_rbin + 1] int32 (the module's docstring), ``wind_thresholds``,
    ``rain_thresholds``, and with ``return_values`` ``site_wind`` and ``site_rain`` (or ``site_peak_rate``) [n_site][n_trk]: bit
    for bit windfield.site_wind's ``site_max`` and rainfall.site_rain's values where a storm's eight planes are finite as far as
    the planes either of them reads.
    """
    wplanes, fl, wthr, wprm = windfield._prepare((lon, lat, v, env), dt_s, rmax_km, ck_cd, wind_r_out_km, substeps, wind_thresholds,
                                                 n_groups)
    rplanes, _, rthr, rprm, _ = rainfall._prepare((lon, lat, vmax), dt_s, stat, rain_r_out_km, substeps, coefficients, v_lo_kt, v_hi_kt,
                                                  rain_thresholds, n_groups)
    n_wbin, n_rbin = int(wthr.size), int(rthr.size)
    if (n_wbin + 1) * (n_rbin + 1) > MAX_CELLS:
        raise ValueError('(n_wbin + 1) * (n_rbin + 1) must be <= %d' % MAX_CELLS)
    planes = wplanes[:7] + [rplanes[2]] + wplanes[7:]      # the footprint's seven, vmax, then the rmax_km plane when there is one

    def make_args(a):
        p = a.planes + [None]                               # (no rmax_km plane)
        trk = _lib.WindTracks(lon=p[0], lat=p[1], v=p[2], u250=p[3], v250=p[4], u850=p[5], v850=p[6], rmax_km=p[8], **a.tracks)
        _, wthr_p, counts, site_wind = a.out
        return (C.byref(trk), p[7], C.byref(wprm), C.byref(rprm)) + a.sites + \
            (n_wbin, wthr_p, n_rbin, rthr.ctypes.data_as(_lib.DP), counts, site_wind, a.outputs[0] if a.outputs else None)
    res = site_scan('tcr_compound', planes, fl, groups, n_groups, site_lon, site_lat, wthr, return_values, engine, device, make_args,
                    more_outputs=(('site_rain', 'pair'),) if return_values else (), count_cells=(n_wbin + 1) * (n_rbin + 1))
    c = res['counts']
    out = dict(counts=c.reshape(c.shape[0], c.shape[1], n_wbin + 1, n_rbin + 1), wind_thresholds=wthr, rain_thresholds=rthr)
    if return_values:
        out['site_wind'] = res['site_max']
        out[RAIN_KEY[stat]] = res['site_rain']
    return out


def or_counts(counts):
    """[..., n_wbin][n_rbin]: the number of storms with W >= wind_thresholds[a] or P >= rain_thresholds[b], from site_compound's
    ``counts`` by inclusion-exclusion (wind + rain - both)."""
    return counts[..., 1:, :1] + counts[..., :1, 1:] - counts[..., 1:, 1:]


def table_return_periods(table, total_years):
    """hazard.return_periods of a [n_site][n_group][n_wbin][n_rbin] table of counts: [n_site][n_wbin][n_rbin] years."""
    t = analysis.to_numpy(table)
    return hazard.return_periods(t.reshape(t.shape[0], t.shape[1], -1), total_years).reshape(t.shape[0], t.shape[2], t.shape[3])


# ---------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.compound',
                                description='Joint (wind and rain) and either (wind or rain) exceedance counts and return periods '
                                            'of track files at sites.')
    analysis.add_site_args(p)
    p.add_argument('--wind-thresholds', type=lambda t: analysis.parse_range(t, '--wind-thresholds'), default=DEFAULT_WIND_THRESHOLDS,
                   metavar='LO:HI:STEP', help='m/s; default %s' % ' '.join('%g' % t for t in DEFAULT_WIND_THRESHOLDS))
    p.add_argument('--rain-thresholds', type=lambda t: analysis.parse_range(t, '--rain-thresholds'), default=None, metavar='LO:HI:STEP',
                   help='mm (total) or mm/h (peak-rate); default for total: %s' % ' '.join('%g' % t for t in DEFAULT_RAIN_THRESHOLDS))
    p.add_argument('--wind-r-out-km', type=float, default=500.0)
    p.add_argument('--rain-r-out-km', type=float, default=500.0)
    p.add_argument('--substeps', type=int, default=1, help='evaluation points per sample interval (1 = the samples only)')
    p.add_argument('--stat', choices=sorted(rainfall.STATS), default='total', help='total: mm per storm; peak-rate: mm/h (needs --rain-thresholds)')
    p.add_argument('--rmax-km', type=float, default=None, help='constant radius of maximum wind (default: Willoughby et al. 2006)')
    p.add_argument('--ck-cd', type=float, default=None, help='Ck / Cd of the profile (default: the namelist\'s)')
    analysis.add_track_args(p, 'compound.npz')
    a = analysis.finish_parse(p, p.parse_args(argv))
    if a.rain_thresholds is None:
        if a.stat != 'total':
            p.error('--stat peak-rate needs --rain-thresholds (mm/h)')
        a.rain_thresholds = DEFAULT_RAIN_THRESHOLDS
    if (len(a.wind_thresholds) + 1) * (len(a.rain_thresholds) + 1) > MAX_CELLS:
        p.error('(wind thresholds + 1) x (rain thresholds + 1) must be <= %d' % MAX_CELLS)
    return a


def main(argv=None):
    args = parse_args(argv)
    inp = analysis.load_inputs(args, wind=True)
    site_lon, site_lat, total_years = inp.site_lon, inp.site_lat, inp.total_years
    res = site_compound(inp.lon, inp.lat, inp.v, inp.vmax, inp.env, inp.groups, site_lon, site_lat, inp.dt_s, args.wind_thresholds,
                        args.rain_thresholds, rmax_km=args.rmax_km, ck_cd=args.ck_cd, wind_r_out_km=args.wind_r_out_km,
                        rain_r_out_km=args.rain_r_out_km, substeps=args.substeps, stat=args.stat, device=args.device,
                        n_groups=total_years)
    counts = res['counts']
    joint = table_return_periods(counts[:, :, 1:, 1:], total_years)
    either = table_return_periods(or_counts(counts), total_years)
    analysis.save_npz(args, inp, dict(counts=counts, joint_return_period=joint, either_return_period=either,
                                      wind_thresholds=res['wind_thresholds'], rain_thresholds=res['rain_thresholds'],
                                      wind_r_out_km=args.wind_r_out_km, rain_r_out_km=args.rain_r_out_km, stat=args.stat),
                      recorded=('substeps', 'rmax_km'))
    analysis.print_summary(args, inp, ', wind r_out = %g km, rain (%s) r_out = %g km, %d substeps'
                           % (args.wind_r_out_km, args.stat, args.rain_r_out_km, args.substeps))
    if site_lon.size <= 10:
        unit = 'mm' if args.stat == 'total' else 'mm/h'
        analysis.print_site_tables('joint return period (years): rows wind (m/s), columns rain (%s): ' % unit
                                   + ' '.join('%6g' % t for t in res['rain_thresholds']), site_lon, site_lat,
                                   ['%6g: ' % u for u in res['wind_thresholds']], joint, '%6.3g')
    return 0


if __name__ == '__main__':
    sys.exit(main())
