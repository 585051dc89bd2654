"""Site wind hazard: near-site intensity, exceedance counts and return periods of a track ensemble.

The analysis of the reference's ``notebooks/sample_analysis.ipynb``, for many sites at once and on the GPU
(``csrc/tcr_hazard.hip``):

1. for each storm, the maximum ``vmax_trks`` over its samples within ``radius_km`` (the notebook's haversine,
   r_earth = 6378 km) of a site (NaN when there are none);
2. per group of storms (a year, or an (ensemble file, year) pair), the number of storms whose value is ``>= v`` for
   ascending thresholds ``v``;
3. the return period ``total_years / exceedance_count`` (``inf`` where the count is 0).

    python -m tropical_cyclone_risk_amd.hazard TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --out hazard.npz

With ``--return-periods 10,50,100`` also the inverse, the near-site intensity of those return periods at every site (levels.py);
with ``--tail-exceedances K`` on top, also their levels from a tail fitted to the site's K largest storms (``levels.row_tail``).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis
from .analysis import DEFAULT_THRESHOLDS, collect_sites, load_groups, read_sites_csv  # noqa: F401
from .basins import BASIN_IDS
from .sitescan import site_scan


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
    planes, fl = analysis.as_planes((lon, lat, vmax), 'lon, lat and vmax')
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))

    def make_args(a):
        lon_, lat_, vmax_ = a.planes
        return (C.byref(_lib.HazardTracks(lon=lon_, lat=lat_, vmax=vmax_, **a.tracks)),) + a.sites + (float(radius_km),) + a.out
    return site_scan('tcr_hazard', planes, fl, groups, n_groups, site_lon, site_lat, thr, return_max, engine, device, make_args)


def return_periods(counts, total_years):
    """total_years / exceedance count (the notebook's formula), ``inf`` where the count is 0.  counts: [..][n_group][n_bin]
    (summed over groups) or [n_site][n_bin] already summed (2-D)."""
    c = analysis.to_numpy(counts)
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
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.hazard',
                                description='Near-site intensity exceedance counts and return periods of track files.')
    analysis.add_site_args(p)
    p.add_argument('--radius-km', type=float, default=100.0)
    analysis.add_threshold_arg(p)
    analysis.add_return_period_arg(p, 'near-site intensity (m/s)')
    analysis.add_events_arg(p, 'near-site intensity (m/s)')
    analysis.add_track_args(p, 'hazard.npz')
    return analysis.finish_parse(p, p.parse_args(argv))


def main(argv=None):
    args = parse_args(argv)
    inp = analysis.load_inputs(args, spacing=False)
    kw = dict(radius_km=args.radius_km, thresholds=args.thresholds, n_groups=inp.total_years)

    def block(t, x, y, plane=False, device=0):
        return site_hazard(t[0], t[1], t[2], inp.groups, x, y, return_max=plane, device=device, **kw)
    return analysis.threshold_main(args, inp, block, (inp.lon, inp.lat, inp.vmax), 'site_max', arrays=dict(radius_km=args.radius_km))


if __name__ == '__main__':
    sys.exit(main())
