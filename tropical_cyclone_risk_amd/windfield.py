"""Wind footprints: the peak wind every storm of a track ensemble produces at every site, and its return periods.

Each sample of a track is a vortex: the Emanuel & Rotunno (2011) radial profile of the azimuthal-mean wind ``v_trks`` around the
centre, with radius of maximum wind ``rm`` (given, or Willoughby, Darling & Rahn 2006), plus the asymmetry of the model's own
``axi_to_max_wind`` (translation speed and shear, ``wind/tc_wind.py``), so that at ``r = rm`` on the azimuth of maximum wind the
footprint is the pipeline's ``vmax_trks``.  On the GPU (``csrc/tcr_windfield.hip``), for many sites at once:

1. for each storm, the maximum over its samples (and linear sub-samples between them) within ``r_out_km`` of a site of the wind
   that sample produces there (NaN when there are none);
2. per group of storms (a year, or an (ensemble file, year) pair), the number of storms whose peak is ``>= v`` for ascending
   thresholds ``v``;
3. the return period ``total_years / exceedance_count`` (``hazard.return_periods``).

The contract is the header's "wind footprint" section (include/tcrisk_hip.h).

    python -m tropical_cyclone_risk_amd.windfield TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --out wind.npz

With ``--return-periods 10,50,100`` also the inverse, the peak wind of those return periods at every site (levels.py); with
``--tail-exceedances K`` on top, also their levels from a generalized Pareto tail fitted to the site's K largest storms, which
reach past the record (``levels.row_tail``).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis, sitescan
from .analysis import DEFAULT_THRESHOLDS, ENV_VARS  # noqa: F401
from .sitescan import MAX_R_OUT_KM, MAX_SUBSTEPS, site_scan  # noqa: F401


def _default_ck_cd():
    from . import namelist
    return float(namelist.Ck) / float(namelist.Cd)


def _track_length(planes, xp):
    """[n_trk] length of the leading run of samples where every plane is finite."""
    fin = planes[0] == planes[0]
    for p in planes:
        fin = fin & xp.isfinite(p)
    n_t = int(fin.shape[1])
    if xp is np:
        return np.where(fin.all(axis=1), n_t, np.argmin(fin, axis=1))
    f = fin.to(xp.int8)
    return xp.where(fin.all(dim=1), xp.full_like(f[:, 0], n_t, dtype=xp.int64), f.argmin(dim=1))


def site_wind(lon, lat, v, env, groups, site_lon, site_lat, dt_s, rmax_km=None, ck_cd=None, r_out_km=500., substeps=1,
              thresholds=DEFAULT_THRESHOLDS, return_max=False, engine=None, device=0, n_groups=None):
    """Peak footprint wind and exceedance counts of every site.

    lon, lat, v: [n_trk][n_t] fp64 (the track file's lon_trks, lat_trks, v_trks); env: (u250, v250, u850, v850), each [n_trk][n_t]
    (the file's *_trks).  A storm's track is its leading run of samples where all seven are finite.  NumPy arrays or torch
    tensors on the GPU (then everything stays there).  dt_s: the sample spacing (s).  rmax_km: None (Willoughby et al. 2006 from v
    and lat), a scalar, or a [n_trk][n_t] plane (km, > 0 and finite on every track sample).  ck_cd: Ck / Cd of the profile, in
    (0, 2) (None: the namelist's).  r_out_km: samples farther from a site do not count there, in (0, 2000].  substeps: 1..64
    evaluation points per sample interval (linear sub-samples between samples).  groups, n_groups, site_lon / site_lat,
    thresholds, return_max, engine, device: as hazard.site_hazard.  Returns a dict: ``counts`` [n_site][n_groups][n_bin] int32,
    ``thresholds``, and with ``return_max`` ``site_max`` [n_site][n_trk] (m/s; NaN: no sample within r_out_km), in the type and
    on the device of ``lon``.
    """
    planes, fl, thr, prm = _prepare((lon, lat, v, env), dt_s, rmax_km, ck_cd, r_out_km, substeps, thresholds, n_groups)

    def make_args(a):
        return (C.byref(_tracks_struct(a)), C.byref(prm)) + a.sites + a.out
    return site_scan('tcr_windfield', planes, fl, groups, n_groups, site_lon, site_lat, thr, return_max, engine, device, make_args)


def _tracks_struct(a):
    """tcr_wind_tracks of site_scan's ScanArgs (seven planes, or eight with rmax_km)."""
    p = a.planes + [None]                                  # (no rmax_km plane)
    return _lib.WindTracks(lon=p[0], lat=p[1], v=p[2], u250=p[3], v250=p[4], u850=p[5], v850=p[6], rmax_km=p[7], **a.tracks)


def _prepare(tracks, dt_s, rmax_km, ck_cd, r_out_km, substeps, thresholds, n_groups):
    """The footprint's argument checks (ValueError, before the library is touched): (planes, their analysis.Flavour, thresholds,
    tcr_wind_params), shared with the analyses built on the footprint.  tracks: (lon, lat, v, env)."""
    lon, lat, v, env = tracks
    if len(env) != 4:
        raise ValueError('env must be (u250, v250, u850, v850)')
    planes, fl = analysis.as_planes((lon, lat, v) + tuple(env), 'lon, lat, v and the four env planes')
    xp = fl.xp
    n_trk, n_t = int(planes[0].shape[0]), int(planes[0].shape[1])
    if n_t < 1:
        raise ValueError('the tracks need at least one sample')
    dt_s = sitescan.check_dt(dt_s)
    ck_cd = _default_ck_cd() if ck_cd is None else float(ck_cd)
    if not 0.0 < ck_cd < 2.0:
        raise ValueError('ck_cd must be in (0, 2)')
    r_out_km = sitescan.check_r_out(r_out_km)
    substeps = sitescan.check_substeps(substeps)
    thr = sitescan.check_ascending(thresholds, sitescan.BOUNDED_THRESHOLDS, max_size=sitescan.MAX_CELLS)
    rm_const = 0.0
    if rmax_km is not None:
        if np.ndim(analysis.to_numpy(rmax_km)) == 0:
            rm_const = float(rmax_km)
            if not (np.isfinite(rm_const) and rm_const > 0):
                raise ValueError('rmax_km must be finite and > 0')
        else:
            rm_plane = fl.conv(rmax_km)
            if tuple(rm_plane.shape) != (n_trk, n_t):
                raise ValueError('an rmax_km plane must be [n_trk][n_t]')
            n = _track_length(planes, xp)
            ar = xp.arange(n_t, device=planes[0].device)[None, :] if xp is not np else np.arange(n_t)[None, :]
            used = (ar < n[:, None]) & (n[:, None] >= 2)
            ok = xp.isfinite(rm_plane) & (rm_plane > 0)
            if bool((used & ~ok).any()):
                raise ValueError('rmax_km must be finite and > 0 at every sample of a track')
            planes.append(rm_plane)
    sitescan.check_n_groups(n_groups)
    return planes, fl, thr, _lib.WindParams(dt_s=dt_s, ck_cd=ck_cd, r_out_km=r_out_km, rmax_const_km=rm_const, substeps=substeps)


# ---------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.windfield',
                                description='Wind-footprint exceedance counts and return periods of track files at sites.')
    analysis.add_site_args(p)
    analysis.add_footprint_args(p)
    analysis.add_threshold_arg(p)
    analysis.add_return_period_arg(p, 'peak wind (m/s)')
    analysis.add_events_arg(p, 'peak wind (m/s)')
    analysis.add_track_args(p, 'wind.npz')
    return analysis.finish_parse(p, p.parse_args(argv))


def main(argv=None):
    args = parse_args(argv)
    inp = analysis.load_inputs(args, wind=True)
    kw = dict(rmax_km=args.rmax_km, ck_cd=args.ck_cd, r_out_km=args.r_out_km, substeps=args.substeps, thresholds=args.thresholds,
              n_groups=inp.total_years)

    def block(t, x, y, plane=False, device=0):
        return site_wind(t[0], t[1], t[2], t[3], inp.groups, x, y, inp.dt_s, return_max=plane, device=device, **kw)
    return analysis.threshold_main(args, inp, block, (inp.lon, inp.lat, inp.v, tuple(inp.env)), 'site_max',
                                   recorded=('r_out_km', 'substeps', 'rmax_km'),
                                   middle=', r_out = %g km, %d substeps' % (args.r_out_km, args.substeps))


if __name__ == '__main__':
    sys.exit(main())
