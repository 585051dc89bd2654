"""Portfolio loss: what a track ensemble costs a set of exposed values, from the wind footprint and a damage function.

For site ``i`` with exposed value ``value[i]`` and storm ``s`` with footprint peak wind ``m`` there (``windfield.site_wind``'s
``site_max``; NaN when the storm never comes within ``r_out_km``), the Emanuel (2011) damage function with CLIMADA's default
constants gives

    x = max(m - v_thresh, 0) / (v_half_i - v_thresh),    D = x^3 / (1 + x^3),    loss[i][s] = value[i] * D    (0 when m is NaN)

On the GPU (``csrc/tcr_loss.hip``) the losses are summed over the sites inside the footprint scan, so the [n_site][n_trk] matrix
never exists:

1. ``event_loss`` [n_trk]: the loss of every storm over the portfolio (the event loss table);
2. ``year_agg`` / ``year_max`` [n_group]: the sum and the largest of the event losses of every group (a year, or an (ensemble
   file, year) pair);
3. ``site_loss`` [n_site]: the loss of every site over all storms (divided by the years: a loss-cost map);
4. the footprint's exceedance ``counts``, which the scan computes anyway.

``loss_curve`` turns the year losses into the aggregate (AEP, from ``year_agg``) or occurrence (OEP, from ``year_max``) loss at
given return periods, ``average_annual_loss`` into the AAL.  The contract is the header's "portfolio loss" section
(include/tcrisk_hip.h).

    python -m tropical_cyclone_risk_amd.loss TRACKS.nc [TRACKS_e0.nc ...] --exposure FILE.csv --out loss.npz
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis, windfield
from .analysis import DEFAULT_THRESHOLDS, to_numpy
from .levels import DEFAULT_RETURN_PERIODS, ranks_of_periods
from .sitescan import site_scan

V_THRESH, V_HALF = 25.7, 74.7          # m/s: CLIMADA's defaults of the Emanuel (2011) function


def damage(m, v_thresh=V_THRESH, v_half=V_HALF):
    """The damage fraction D of peak wind m (NumPy, broadcast): 0 at and below v_thresh and at NaN, 1/2 at v_half, -> 1."""
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        x = np.where(np.isnan(m), 0.0, np.maximum(m - v_thresh, 0.0)) / (np.asarray(v_half, dtype=np.float64) - v_thresh)
        x3 = x * x * x
        return np.where(np.isfinite(x3), x3 / (1.0 + x3), 1.0)


def portfolio_loss(lon, lat, v, env, groups, site_lon, site_lat, value, dt_s, v_thresh=V_THRESH, v_half=V_HALF, rmax_km=None,
                   ck_cd=None, r_out_km=500., substeps=1, thresholds=DEFAULT_THRESHOLDS, engine=None, device=0,
                   n_groups=None):
    """Event losses, year losses, site losses and footprint exceedance counts of a portfolio.

    lon, lat, v, env, groups, n_groups, site_lon / site_lat, dt_s, rmax_km, ck_cd, r_out_km, substeps, thresholds, engine,
    device: as windfield.site_wind (NumPy arrays, or torch tensors on the GPU: then everything stays there).  value: [n_site]
    exposed value of every site, finite and >= 0.  v_thresh: finite, >= 0 (m/s).  v_half: a scalar or one value per site, finite
    and > v_thresh.  Returns a dict: ``event_loss`` [n_trk] in the caller's storm order, ``year_agg`` and ``year_max``
    [n_groups] (0 for a group without storms), ``site_loss`` [n_site] and ``counts`` [n_site][n_groups][n_bin] int32 in the
    caller's site order, ``thresholds``; arrays in the type and on the device of ``lon``.  No sum uses atomics: a repeated call
    gives the same bits.
    """
    planes, fl, thr, wprm = windfield._prepare((lon, lat, v, env), dt_s, rmax_km, ck_cd, r_out_km, substeps, thresholds, n_groups)
    xp, conv = fl.xp, fl.conv
    v_thresh = float(v_thresh)
    if not (np.isfinite(v_thresh) and v_thresh >= 0):
        raise ValueError('v_thresh must be finite and >= 0')
    value = conv(value).reshape(-1)
    n_site = int(conv(site_lon).reshape(-1).shape[0])
    if value.shape[0] != n_site:
        raise ValueError('value must hold one number per site')
    if not bool((xp.isfinite(value) & (value >= 0)).all()):
        raise ValueError('value must be finite and >= 0')
    vh_site = None
    if np.ndim(to_numpy(v_half)) == 0:
        vh0 = float(v_half)
        if not (np.isfinite(vh0) and vh0 > v_thresh):
            raise ValueError('v_half must be finite and > v_thresh')
    else:
        vh_site = conv(v_half).reshape(-1)
        if vh_site.shape[0] != n_site:
            raise ValueError('a per-site v_half must hold one number per site')
        if not bool((xp.isfinite(vh_site) & (vh_site > v_thresh)).all()):
            raise ValueError('v_half must be finite and > v_thresh at every site')
        vh0 = float(vh_site.max()) if n_site else V_HALF      # (the scalar is not used, but it is checked)
    lprm = _lib.LossParams(v_thresh=v_thresh, v_half=vh0)

    def make_args(a):
        return (C.byref(windfield._tracks_struct(a)), C.byref(wprm), C.byref(lprm)) + a.sites + tuple(a.extras) + a.out[:3] + \
            tuple(a.outputs)
    return site_scan('tcr_loss', planes, fl, groups, n_groups, site_lon, site_lat, thr, False, engine, device, make_args,
                     site_extras=(value, vh_site),
                     more_outputs=(('event_loss', 'trk'), ('year_agg', 'group'), ('year_max', 'group'), ('site_loss', 'site')))


def year_loss_table(event_loss, groups, n_groups):
    """(year_agg, year_max) [n_groups] of an event loss table in NumPy: the sum and the largest event loss of every group, 0 for
    a group without storms.  For callers who filter or rescale events first."""
    e = to_numpy(event_loss).astype(np.float64).reshape(-1)
    bad = 'groups must hold one integer in [0, n_groups) per event'
    g, n_groups = analysis.group_index(groups, e.shape[0], int(n_groups), bad=bad, over=bad)
    if n_groups < 1:
        raise ValueError(bad)
    agg, mx = np.zeros(n_groups), np.zeros(n_groups)
    if e.size:
        np.add.at(agg, g, e)
        np.maximum.at(mx, g, e)
    return agg, mx


def loss_curve(year_losses, total_years, return_periods=DEFAULT_RETURN_PERIODS):
    """The loss at every return period T: the k-th largest year loss, k the smallest integer with k * T >= total_years (the loss
    exceeded or equalled in k of total_years years has the return period total_years / k, hazard.return_periods' formula).
    NaN for T > total_years, the smallest year loss for T < 1; years beyond len(year_losses) count as 0.  year_agg gives the
    aggregate (AEP) curve, year_max the occurrence (OEP) curve."""
    y = to_numpy(year_losses).astype(np.float64).reshape(-1)
    total_years = int(total_years)
    if total_years < 1 or y.size > total_years:
        raise ValueError('total_years must be >= 1 and >= the number of year losses')
    k, defined = ranks_of_periods(return_periods, total_years)
    desc = np.zeros(total_years)
    desc[:y.size] = np.sort(y)[::-1]
    return np.where(defined, desc[np.clip(k, 1, total_years) - 1], np.nan)


def average_annual_loss(year_agg, total_years):
    """The sum of the year losses over total_years (years beyond len(year_agg) count as 0)."""
    y = to_numpy(year_agg).astype(np.float64)
    return float(y.sum() / float(total_years))


# ---------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.loss',
                                description='Event, year and site losses and AEP / OEP loss curves of track files for an exposure.')
    p.add_argument('--exposure', required=True, metavar='FILE.csv',
                   help='one LON,LAT,VALUE[,V_HALF] per line (lines that are not numbers are skipped)')
    p.add_argument('--v-thresh', type=float, default=V_THRESH, help='wind below which nothing is damaged (m/s)')
    p.add_argument('--v-half', type=float, default=V_HALF, help='wind of half damage (m/s) where the exposure gives none')
    analysis.add_footprint_args(p)
    p.add_argument('--return-periods', type=analysis.parse_periods, default=np.array(DEFAULT_RETURN_PERIODS), metavar='T1,T2,...')
    analysis.add_track_args(p, 'loss.npz')
    return p.parse_args(argv)


def read_exposure_csv(fn, v_half=V_HALF):
    """lon, lat, value, v_half [n] of LON,LAT,VALUE[,V_HALF] lines; v_half where a line has no fourth column.  The last element
    tells whether any line had one."""
    rows, any_vh = [], False
    for line in open(fn):
        f = [x for x in line.replace(';', ',').split(',')]
        try:
            if len(f) >= 3:
                row = [float(f[0]), float(f[1]), float(f[2])]
                has = len(f) >= 4 and f[3].strip() != ''
                row.append(float(f[3]) if has else float(v_half))
                rows.append(row)
                any_vh = any_vh or has
        except ValueError:
            pass
    a = np.array(rows, dtype=np.float64).reshape(-1, 4)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(), any_vh


def main(argv=None):
    args = parse_args(argv)
    site_lon, site_lat, value, vh, any_vh = read_exposure_csv(args.exposure, args.v_half)
    if site_lon.size == 0:
        raise SystemExit('no exposure')
    inp = analysis.load_inputs(args, wind=True, sites=(site_lon, site_lat))
    total_years = inp.total_years
    res = portfolio_loss(inp.lon, inp.lat, inp.v, inp.env, inp.groups, site_lon, site_lat, value, inp.dt_s, v_thresh=args.v_thresh,
                         v_half=vh if any_vh else args.v_half, rmax_km=args.rmax_km, ck_cd=args.ck_cd, r_out_km=args.r_out_km,
                         substeps=args.substeps, device=args.device, n_groups=total_years)
    T = args.return_periods
    aal = average_annual_loss(res['year_agg'], total_years)
    aep, oep = loss_curve(res['year_agg'], total_years, T), loss_curve(res['year_max'], total_years, T)
    analysis.save_npz(args, inp, dict(event_loss=res['event_loss'], year_agg=res['year_agg'], year_max=res['year_max'],
                                      site_loss=res['site_loss'], loss_cost=res['site_loss'] / total_years, counts=res['counts'],
                                      thresholds=res['thresholds'], aal=aal, return_periods=T, aep=aep, oep=oep, value=value, v_half=vh,
                                      v_thresh=args.v_thresh), recorded=('r_out_km', 'substeps', 'rmax_km'))
    analysis.print_summary(args, inp, ', r_out = %g km, %d substeps' % (args.r_out_km, args.substeps),
                           site_note=' (total value %g)' % value.sum())
    print('average annual loss: %.6g' % aal)
    print('return period (years):      ' + ' '.join('%10g' % t for t in T))
    print('aggregate loss (AEP):       ' + ' '.join('%10.4g' % x for x in aep))
    print('occurrence loss (OEP):      ' + ' '.join('%10.4g' % x for x in oep))
    return 0


if __name__ == '__main__':
    sys.exit(main())
