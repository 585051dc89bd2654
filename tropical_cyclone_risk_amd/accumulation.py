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
MAX_CELLS = sitescan.MAX_CELLS
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
    scan = _bind(groups, dt_s, windows_h, thresholds, r_out_km, substeps, coefficients, v_lo_kt, v_hi_kt, n_groups)
    res, fl = scan((lon, lat, vmax), site_lon, site_lat, return_values, engine, device)
    return sitescan.attach_planes(res, fl, 'site_window', return_values, lon)


def _check_windows(windows_h, dt_s, thresholds, return_values):
    """The accumulation's own argument checks (ValueError): (windows_h, window_samples int32, the sorted window indices whose
    planes are wanted)."""
    try:
        dt = sitescan.check_dt(dt_s)
    except (TypeError, ValueError):                         # (a dt_s that is no number at all gets the same text here)
        raise ValueError(sitescan.BAD_DT)
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
    thr = sitescan.check_ascending(thresholds, sitescan.ASCENDING % 'thresholds')
    if m.size * (thr.size + 1) > MAX_CELLS:
        raise ValueError('n_window * (n_bin + 1) must be <= %d' % MAX_CELLS)
    if 512 * (int(m[-1]) + 1) + 256 * m.size * (thr.size + 1) > MAX_LDS:
        raise ValueError('512 (longest window in samples + 1) + 256 n_window (n_bin + 1) must be <= %d' % MAX_LDS)
    return win_h, m, sitescan.wanted_rows(return_values, m.size, 'return_values', 'window')


def _bind(groups, dt_s, windows_h, thresholds, r_out_km=500., substeps=1, coefficients=None, v_lo_kt=35., v_hi_kt=155., n_groups=None):
    """site_accumulation's arguments, checked as far as they stand alone (_check_windows) and bound into sitescan's
    scan(tracks = (lon, lat, vmax), site_lon, site_lat, want, engine, device): one call of tcr_accumulation_*, whose ``planes`` are
    those of the windows in want (a return_values).  rainfall._prepare needs the tracks: it runs in every call, after want's check."""
    win_h, m, _ = _check_windows(windows_h, dt_s, thresholds, False)
    n_window = int(m.size)

    def scan(tracks, site_lon, site_lat, want=(), engine=None, device=0):
        want = sitescan.wanted_rows(want, n_window, 'return_values', 'window')
        planes, fl, thr, prm, _ = rainfall._prepare(tracks, dt_s, 'total', r_out_km, substeps, coefficients, v_lo_kt, v_hi_kt,
                                                    thresholds, n_groups)

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
    return scan


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
    a = analysis.finish_parse(p, p.parse_args(argv), no_tail='--tail-exceedances is not offered for accumulation windows yet')
    if a.windows.size < 1 or not np.isfinite(a.windows).all() or np.any(a.windows <= 0) or np.any(np.diff(a.windows) <= 0) \
            or a.windows.size > MAX_WINDOWS:
        p.error('--windows: 1 to %d positive, strictly ascending window lengths in hours' % MAX_WINDOWS)
    return a


def main(argv=None):
    args = parse_args(argv)
    inp = analysis.load_inputs(args)
    site_lon, site_lat, total_years = inp.site_lon, inp.site_lat, inp.total_years
    tracks = (inp.lon, inp.lat, inp.vmax)
    try:
        scan = _bind(inp.groups, inp.dt_s, args.windows, args.thresholds, r_out_km=args.r_out_km, substeps=args.substeps,
                     n_groups=total_years)
    except ValueError as e:
        raise SystemExit('--windows / --thresholds at the files\' sample spacing of %g s: %s' % (inp.dt_s, e))
    res, _ = scan(tracks, site_lon, site_lat, device=args.device)
    win_h, m = res['windows_h'], res['window_samples']
    more = {}
    if args.return_periods is not None:
        more = sitescan.stacked_return_levels(scan, m.size, tracks, site_lon, site_lat, total_years, args.return_periods, args.device)
    rp = hazard.return_periods(res['counts'], total_years)
    analysis.save_npz(args, inp, dict(counts=res['counts'], return_period=rp, windows_h=win_h, window_samples=m,
                                      thresholds=res['thresholds']), recorded=('r_out_km', 'substeps'), more=more)
    analysis.print_summary(args, inp, ', windows %s h, r_out = %g km, %d substeps'
                           % (','.join('%g' % w for w in win_h), args.r_out_km, args.substeps))
    if site_lon.size <= 10 and more:
        analysis.print_site_tables('rain depth (mm) by window (rows, hours) and return period (years): '
                                   + ' '.join('%8g' % t for t in more['return_periods']), site_lon, site_lat,
                                   ['%6g h: ' % w for w in win_h], more['return_level'], '%8.4g')
    return 0


if __name__ == '__main__':
    sys.exit(main())
