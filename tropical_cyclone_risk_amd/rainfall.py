"""Rainfall footprints: the rain every storm of a track ensemble leaves at every site, and its return periods.

Each sample of a track rains with the R-CLIPER radial profile (Tuleya, DeMaria & Kuligowski 2007) around the centre, a function
of the distance and of ``vmax_trks`` alone, so the three planes every track file has are enough.  On the GPU
(``csrc/tcr_rainfall.hip``), for many sites at once:

1. for each storm, over its samples (and linear sub-samples between them) within ``r_out_km`` of a site, either the time
   integral of the rain rate there (``stat='total'``, mm: the trapezoid rule along the track) or its maximum
   (``stat='peak-rate'``, mm/h); NaN when there are none;
2. per group of storms (a year, or an (ensemble file, year) pair), the number of storms whose value is ``>=`` each of the
   ascending thresholds;
3. the return period ``total_years / exceedance_count`` (``hazard.return_periods``).

The contract is the header's "rainfall footprint" section (include/tcrisk_hip.h).  Not modelled: rain asymmetry from shear or
topography, and decay after landfall.

    python -m tropical_cyclone_risk_amd.rainfall TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --out rain.npz

With ``--return-periods 10,50,100`` also the inverse, the rain of those return periods at every site (levels.py); with
``--tail-exceedances K`` on top, also their levels from a tail fitted to the site's K largest storms (``levels.row_tail``).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis, sitescan
from .sitescan import MAX_R_OUT_KM, MAX_SUBSTEPS, site_scan  # noqa: F401

DEFAULT_RAIN_THRESHOLDS = np.array([25, 50, 75, 100, 150, 200, 250, 300, 400, 500], dtype=np.float64)      # mm
# R-CLIPER, the TRMM fit: T0, Tm (inches/day), rm, re (km) = a + b U
DEFAULT_COEFFICIENTS = ((-1.10, -1.60, 64.5, 150.0), (3.96, 4.80, -13.0, -16.0))
STATS = {'total': (_lib.RAIN_TOTAL, 'site_total'), 'peak-rate': (_lib.RAIN_PEAK_RATE, 'site_peak_rate')}


def site_rain(lon, lat, vmax, groups, site_lon, site_lat, dt_s, stat='total', r_out_km=500., substeps=1, coefficients=None,
              v_lo_kt=35., v_hi_kt=155., thresholds=DEFAULT_RAIN_THRESHOLDS, return_values=False, engine=None, device=0,
              n_groups=None):
    """Storm-total rain (or peak rain rate) and exceedance counts of every site.

    lon, lat, vmax: [n_trk][n_t] fp64 (the track file's lon_trks, lat_trks, vmax_trks).  A storm's track is its leading run of
    samples where all three are finite.  NumPy arrays or torch tensors on the GPU (then everything stays there).  dt_s: the
    sample spacing (s).  stat: 'total' (mm) or 'peak-rate' (mm/h; then thresholds must be given: the defaults are totals).
    r_out_km: samples farther from a site do not count there, in (0, 2000].  substeps: 1..64 evaluation points per sample
    interval.  coefficients: (a, b), four numbers each, of T0, Tm (inches/day), rm and re (km) = a + b U (None: the TRMM fit);
    v_lo_kt, v_hi_kt: the clamp on vmax in knots; rm, re > 0 and Tm >= 0 must hold at both.  groups, n_groups,
    site_lon / site_lat, engine, device: as hazard.site_hazard.  Returns a dict: ``counts`` [n_site][n_groups][n_bin] int32,
    ``thresholds``, and with ``return_values`` ``site_total`` or ``site_peak_rate`` [n_site][n_trk] (NaN: no sample within
    r_out_km), in the type and on the device of ``lon``.
    """
    planes, fl, thr, prm, key = _prepare((lon, lat, vmax), dt_s, stat, r_out_km, substeps, coefficients, v_lo_kt, v_hi_kt, thresholds,
                                         n_groups)

    def make_args(a):
        lon_, lat_, vmax_ = a.planes
        return (C.byref(_lib.HazardTracks(lon=lon_, lat=lat_, vmax=vmax_, **a.tracks)), C.byref(prm)) + a.sites + a.out
    res = site_scan('tcr_rainfall', planes, fl, groups, n_groups, site_lon, site_lat, thr, return_values, engine, device, make_args)
    if return_values:
        res[key] = res.pop('site_max')
    return res


def _prepare(tracks, dt_s, stat, r_out_km, substeps, coefficients, v_lo_kt, v_hi_kt, thresholds, n_groups):
    """The argument checks (ValueError, before the library is touched): (planes, their analysis.Flavour, thresholds,
    tcr_rain_params, the name of the per-storm output).  tracks: (lon, lat, vmax)."""
    planes, fl = analysis.as_planes(tuple(tracks), 'lon, lat and vmax')
    if int(planes[0].shape[1]) < 1:
        raise ValueError('the tracks need at least one sample')
    if stat not in STATS:
        raise ValueError("stat must be 'total' or 'peak-rate'")
    dt_s = sitescan.check_dt(dt_s)
    r_out_km = sitescan.check_r_out(r_out_km)
    substeps = sitescan.check_substeps(substeps)
    if stat == 'peak-rate' and thresholds is DEFAULT_RAIN_THRESHOLDS:       # (by identity: the caller's object, unconverted)
        raise ValueError("stat='peak-rate' needs explicit thresholds (mm/h): the defaults are storm totals in mm")
    thr = sitescan.check_ascending(thresholds, sitescan.BOUNDED_THRESHOLDS, max_size=sitescan.MAX_CELLS)
    try:
        a, b = (np.asarray(c, dtype=np.float64).reshape(-1) for c in (DEFAULT_COEFFICIENTS if coefficients is None else coefficients))
    except (TypeError, ValueError):
        raise ValueError('coefficients must be (a, b), four numbers each')
    if a.size != 4 or b.size != 4 or not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError('coefficients must be (a, b), four finite numbers each')
    v_lo_kt, v_hi_kt = float(v_lo_kt), float(v_hi_kt)
    if not (0.0 < v_lo_kt <= v_hi_kt and np.isfinite(v_hi_kt)):
        raise ValueError('need 0 < v_lo_kt <= v_hi_kt, both finite')
    for kt in (v_lo_kt, v_hi_kt):                           # linear in U: what holds at both ends holds in between
        u = 1.0 + (kt - 35.0) / 33.0
        if not (a[2] + b[2] * u > 0 and a[3] + b[3] * u > 0 and a[1] + b[1] * u >= 0):
            raise ValueError('the coefficients must give rm > 0, re > 0 and Tm >= 0 at v_lo_kt and at v_hi_kt')
    sitescan.check_n_groups(n_groups)
    code, key = STATS[stat]
    prm = _lib.RainParams(dt_s=dt_s, r_out_km=r_out_km, v_lo_kt=v_lo_kt, v_hi_kt=v_hi_kt, a=(C.c_double * 4)(*a),
                          b=(C.c_double * 4)(*b), substeps=substeps, stat=code)
    return planes, fl, thr, prm, key


# ---------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.rainfall',
                                description='Storm-total rainfall (or peak rain rate) exceedance counts and return periods of '
                                            'track files at sites.')
    analysis.add_site_args(p)
    p.add_argument('--stat', choices=sorted(STATS), default='total', help='total: mm per storm; peak-rate: mm/h (needs --thresholds)')
    p.add_argument('--r-out-km', type=float, default=500.0)
    p.add_argument('--substeps', type=int, default=1, help='evaluation points per sample interval (1 = the samples only)')
    p.add_argument('--thresholds', type=lambda t: analysis.parse_range(t, '--thresholds'), default=None, metavar='LO:HI:STEP',
                   help='mm (total) or mm/h (peak-rate); default for total: %s' % ' '.join('%g' % t for t in DEFAULT_RAIN_THRESHOLDS))
    analysis.add_return_period_arg(p, 'storm-total rain (mm) or peak rain rate (mm/h)')
    analysis.add_events_arg(p, 'storm-total rain (mm) or peak rain rate (mm/h)')
    analysis.add_track_args(p, 'rain.npz')
    a = analysis.finish_parse(p, p.parse_args(argv))
    if a.thresholds is None:
        if a.stat != 'total':
            p.error('--stat peak-rate needs --thresholds (mm/h)')
        a.thresholds = DEFAULT_RAIN_THRESHOLDS
    return a


def main(argv=None):
    args = parse_args(argv)
    inp = analysis.load_inputs(args)
    kw = dict(stat=args.stat, r_out_km=args.r_out_km, substeps=args.substeps, thresholds=args.thresholds, n_groups=inp.total_years)

    def block(t, x, y, plane=False, device=0):
        return site_rain(t[0], t[1], t[2], inp.groups, x, y, inp.dt_s, return_values=plane, device=device, **kw)
    return analysis.threshold_main(args, inp, block, (inp.lon, inp.lat, inp.vmax), STATS[args.stat][1],
                                   unit='mm' if args.stat == 'total' else 'mm/h', arrays=dict(stat=args.stat),
                                   recorded=('r_out_km', 'substeps'),
                                   middle=', %s, r_out = %g km, %d substeps' % (args.stat, args.r_out_km, args.substeps))


if __name__ == '__main__':
    sys.exit(main())
