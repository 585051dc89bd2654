"""Rain accumulation windows: the largest rain depth every storm of a track ensemble leaves at every site within any D consecutive
hours, for a few window lengths D at once, how often it reaches given depths, and the depth-duration-frequency (DDF) table of a
site: the D-hour depth of the 10-, 50- and 100-year return period.

The rain is the rainfall footprint's (``rainfall.py``): the same track, records, sub-steps, outer radius and per-pair rate, bit for
bit.  ``site_total`` and ``site_peak_rate`` there are the two ends of one axis, D -> infinity and D -> 0; this is what lies between.
The hourly series of every (site, storm) pair is far too large to store, so the window maximum is formed inside the scan
(``csrc/tcr_accumulation.hip``):

1. with ``h = dt_s / (3600 substeps)`` hours and ``rho_q`` the rate of record ``q`` at the site (0 when the record is farther than
   ``r_out_km``), ``I_q = (h / 2)(rho_q + rho_q+1)`` is the trapezoid of one sub-interval, ``T_k`` the sum of ``I_q`` over
   ``q < k substeps`` (the depth up to sample ``k``) and, for a window of ``m`` samples, ``A = max_k (T_k - T_max(k - m, 0))`` in mm;
   NaN when no record of the storm is within ``r_out_km``;
2. per group of storms (a year, or an (ensemble file, year) pair) and window, the number of storms whose ``A`` is ``>=`` each of
   the ascending thresholds (mm);
3. the return period ``total_years / exceedance_count`` (``hazard.return_periods``).

A window of at least the track's length gives the storm total; ``A`` never decreases with the window's length; and ``A <= D`` times
the peak rate.  The contract is the header's "rain accumulation windows" section (include/tcrisk_hip.h).  Not modelled: windows
start and end on track samples (sub-steps refine the integral inside a sample interval, not the window's position); rain asymmetry
from shear or topography and decay after landfall, as in ``rainfall.py``.

    python -m tropical_cyclone_risk_amd.accumulation TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --windows 6,12,24,48,72

With ``--return-periods 10,50,100`` also the DDF table ``return_level[site][window][T]`` (levels.py).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis, hazard, rainfall
from .rainfall import DEFAULT_RAIN_THRESHOLDS
from . import sitescan

MAX_WINDOWS = 8
MAX_WINDOW_SAMPLES = 96
MAX_CELLS = 64
MAX_LDS = 65536
DEFAULT_WINDOWS_H = (6, 12, 24, 48, 72)


def site_accumulation(lon, lat, vmax, groups, site_lon, site_lat, dt_s, windows_h=DEFAULT_WINDOWS_H, thresholds=DEFAULT_RAIN_THRESHOLDS,
                      return_values=False, r_out_km=500., substeps=1, coefficients=None, v_lo_kt=35., v_hi_kt=155., engine=None,
                      device=0, n_groups=None):
    """Peak rain depth in windows of windows_h hours, and its exceedance counts, at every site.

    lon, lat, vmax, dt_s, r_out_km, substeps, coefficients, v_lo_kt, v_hi_kt, groups, n_groups, site_lon / site_lat, engine, device:
    as rainfall.site_rain, under the same rules.  windows_h: 1 to 8 window lengths in hours, each a whole number of samples
    (windows_h * 3600 / dt_s), positive, strictly ascending, at most 96 samples.  thresholds: depths in mm, finite, strictly
    ascending; n_window * (n_bin + 1) <= 64 and 512 (longest window in samples + 1) + 256 n_window (n_bin + 1) <= 65536.
    return_values: True, or a list of window indices.  Returns a dict: ``counts`` [n_site][n_groups][n_window][n_bin] int32,
    ``windows_h``, ``window_samples``, ``thresholds``, and with ``return_values`` ``site_window`` [n_window][n_site][n_trk] (mm;
    NaN: no sample within r_out_km; all NaN for a window not asked for: a plane is n_site * n_trk * 8 bytes on the device, which
    is why they are selectable), in the type and on the device of ``lon``.
    """
    win_h, m, want = _check_windows(windows_h, dt_s, thresholds, return_values)
    res, fl = _scan(lon, lat, vmax, groups, site_lon, site_lat, dt_s, win_h, m, thresholds, r_out_km, substeps, coefficients, v_lo_kt,
                    v_hi_kt, want, engine, device, n_groups)
    planes = res.pop('planes')
    if return_values is not False and return_values is not None:
        n_trk = int(lon.shape[0]) if hasattr(lon, 'shape') else len(lon)
        res['site_window'] = sitescan.stacked_planes(fl, planes, m.size, int(res['counts'].shape[0]), n_trk)
    return res


def _check_windows(windows_h, dt_s, thresholds, return_values):
    """The accumulation's own argument checks (ValueError): (windows_h, window_samples int32, the sorted window indices whose
    planes are wanted)."""
    try:
        dt = float(dt_s)
    except (TypeError, ValueError):
        raise ValueError('dt_s must be finite and > 0')
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError('dt_s must be finite and > 0')
    win_h = np.ascontiguousarray(np.asarray(windows_h, dtype=np.float64).reshape(-1))
    if not 1 <= win_h.size <= MAX_WINDOWS:
        raise ValueError('give 1 to %d windows' % MAX_WINDOWS)
    if not np.isfinite(win_h).all():
        raise ValueError('windows_h must be finite')
    samples = win_h * 3600.0 / dt
    m = np.rint(samples)
    if np.any(m != samples):
        raise ValueError('every window must be a whole number of samples (windows_h * 3600 / dt_s)')
    if np.any(m < 1) or np.any(m > MAX_WINDOW_SAMPLES) or np.any(np.diff(m) <= 0):
        raise ValueError('windows must be positive, strictly ascending and at most %d samples long' % MAX_WINDOW_SAMPLES)
    m = np.ascontiguousarray(m.astype(np.int32))
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if thr.size < 1 or not np.isfinite(thr).all() or np.any(np.diff(thr) <= 0):
        raise ValueError('thresholds must be finite and strictly ascending')
    if m.size * (thr.size + 1) > MAX_CELLS:
        raise ValueError('n_window * (n_bin + 1) must be <= %d' % MAX_CELLS)
    if 512 * (int(m[-1]) + 1) + 256 * m.size * (thr.size + 1) > MAX_LDS:
        raise ValueError('512 (longest window in samples + 1) + 256 n_window (n_bin + 1) must be <= %d' % MAX_LDS)
    return win_h, m, sitescan.wanted_rows(return_values, m.size, 'return_values', 'window')


def _scan(lon, lat, vmax, groups, site_lon, site_lat, dt_s, win_h, m, thresholds, r_out_km, substeps, coefficients, v_lo_kt, v_hi_kt,
          want, engine, device, n_groups):
    """One call of tcr_accumulation_*: (dict with ``planes`` = {window index: [n_site][n_trk] plane} for the windows in want,
    Flavour)."""
    planes, fl, thr, prm, _ = rainfall._prepare(lon, lat, vmax, dt_s, 'total', r_out_km, substeps, coefficients, v_lo_kt, v_hi_kt,
                                                thresholds, n_groups)
    n_window = int(m.size)

    def make_args(a, win):
        lon_, lat_, vmax_ = a.planes
        n_bin_, thr_, counts_, _ = a.out
        return (C.byref(_lib.HazardTracks(lon=lon_, lat=lat_, vmax=vmax_, **a.tracks)), C.byref(prm)) + a.sites + \
            (n_window, m.ctypes.data_as(C.POINTER(C.c_int32)), n_bin_, thr_, counts_, win)
    res = sitescan.stacked_scan('tcr_accumulation', planes, fl, groups, n_groups, site_lon, site_lat, thr, n_window, want, 'window',
                                engine, device, make_args)
    res['windows_h'] = win_h
    res['window_samples'] = m
    return res, fl


# ---------------------------------------------------------------------------------------------------------------- CLI
def _parse_windows(text):
    try:
        return np.array([float(x) for x in text.split(',')])
    except ValueError:
        raise argparse.ArgumentTypeError('--windows: expected H1,H2,... (hours), got %r' % text)


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.accumulation',
                                description='Peak rain depth in windows of D hours at sites: exceedance counts, their return periods '
                                            'and the depth-duration-frequency table.')
    analysis.add_site_args(p)
    p.add_argument('--windows', type=_parse_windows, default=np.array(DEFAULT_WINDOWS_H, dtype=np.float64), metavar='H1,H2,...',
                   help='1 to 8 ascending window lengths in hours, whole numbers of samples (default: %s)'
                        % ','.join('%g' % w for w in DEFAULT_WINDOWS_H))
    p.add_argument('--r-out-km', type=float, default=500.0)
    p.add_argument('--substeps', type=int, default=1, help='evaluation points per sample interval (1 = the samples only)')
    p.add_argument('--thresholds', type=lambda t: analysis.parse_range(t, '--thresholds'), default=DEFAULT_RAIN_THRESHOLDS,
                   metavar='LO:HI:STEP', help='depths in mm (default: %s)' % ' '.join('%g' % t for t in DEFAULT_RAIN_THRESHOLDS))
    analysis.add_return_period_arg(p, 'the rain depth of every window (mm)')
    analysis.add_track_args(p, 'accumulation.npz')
    a = p.parse_args(argv)
    if a.tail_exceedances is not None:
        p.error('--tail-exceedances is not offered for accumulation windows yet')
    if not (a.site or a.sites or a.grid):
        p.error('give sites with --site, --sites or --grid')
    if a.windows.size < 1 or not np.isfinite(a.windows).all() or np.any(a.windows <= 0) or np.any(np.diff(a.windows) <= 0) \
            or a.windows.size > MAX_WINDOWS:
        p.error('--windows: 1 to %d positive, strictly ascending window lengths in hours' % MAX_WINDOWS)
    return a


def main(argv=None):
    args = parse_args(argv)
    site_lon, site_lat = analysis.collect_sites(args)
    if site_lon.size == 0:
        raise SystemExit('no sites')
    lon, lat, vmax, groups, gfile, gyear, more = analysis.load_groups(args.tracks, extra=('time',))
    dt = analysis.sample_spacing(more['time'])
    total_years = len(gfile)
    try:
        win_h, m, _ = _check_windows(args.windows, dt, args.thresholds, False)
    except ValueError as e:
        raise SystemExit('--windows / --thresholds at the files\' sample spacing of %g s: %s' % (dt, e))
    kw = dict(r_out_km=args.r_out_km, substeps=args.substeps, n_groups=total_years)
    res = site_accumulation(lon, lat, vmax, groups, site_lon, site_lat, dt, windows_h=win_h, thresholds=args.thresholds,
                            device=args.device, **kw)
    more = {}
    if args.return_periods is not None:
        def one(i, t, x, y):
            r, _ = _scan(t[0], t[1], t[2], groups, x, y, dt, win_h, m, args.thresholds, kw['r_out_km'], kw['substeps'], None, 35., 155.,
                         [i], None, 0, total_years)
            r['value'] = r.pop('planes')[i]
            return r
        more = sitescan.stacked_return_levels(one, m.size, (lon, lat, vmax), site_lon, site_lat, total_years, args.return_periods,
                                              args.device)
    rp = hazard.return_periods(res['counts'], total_years)
    np.savez(args.out, counts=res['counts'], return_period=rp, windows_h=win_h, window_samples=m, thresholds=res['thresholds'],
             site_lon=site_lon, site_lat=site_lat, total_years=total_years, r_out_km=args.r_out_km, substeps=args.substeps, dt_s=dt,
             **analysis.group_meta(args.tracks, gfile, gyear), **more)
    print('%d sites, %d storms, %d groups (%d files), total_years = %d, windows %s h, r_out = %g km, %d substeps -> %s'
          % (site_lon.size, lon.shape[0], total_years, len(args.tracks), total_years, ','.join('%g' % w for w in win_h), args.r_out_km,
             args.substeps, args.out))
    if site_lon.size <= 10 and more:
        print('rain depth (mm) by window (rows, hours) and return period (years): ' + ' '.join('%8g' % t for t in more['return_periods']))
        for s in range(site_lon.size):
            print('  site (%.4f, %.4f)' % (site_lon[s], site_lat[s]))
            for i, w in enumerate(win_h):
                print('    %6g h: ' % w + ' '.join('%8.4g' % x for x in more['return_level'][s, i]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
