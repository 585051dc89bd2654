"""Closest approach: how every storm of a track ensemble passed every site.  The distance of the closest point of approach (CPA),
when it happened, how strong the storm was, how fast and where to it was moving, its radius of maximum wind and the side of the
track the site was on; and how often storms pass within each of a few distance bands at or above given intensities, the statistic
behind "hurricanes passing within 50 nmi" and the joint-probability method of coastal-surge work.

Every other site analysis here reduces a storm to one extreme at a site; ``hazard`` is the nearest, the maximum intensity anywhere
within a radius, and says nothing about the geometry.  On the GPU (``csrc/tcr_approach.hip``), for many sites at once:

1. a storm's records are its samples and ``substeps - 1`` linear sub-samples between neighbours (the wind footprint's, longitude the
   short way round); a record moves as the segment it lies on does (``ue``, ``un`` in m/s from the segment's ends, the track's last
   record takes the last segment's; ``heading_deg`` clockwise from north in [0, 360), NaN on a stationary segment);
2. per (site, storm), among the records within the largest band of the site, the one nearest to it, the earliest on a tie, gives
   the seven ``PLANES``; NaN everywhere when no record is that near.  ``side_km`` is ``+distance`` with the site to the right of
   the motion, ``-distance`` to the left, 0.0 when undefined (the site on the centre, a stationary segment);
3. per group of storms (a year, or an (ensemble file, year) pair), band and threshold, the number of storms with
   ``distance_km <= band`` and ``v >= threshold``; the return period is ``total_years / count`` (``hazard.return_periods``).

The contract is the header's "closest approach" section (include/tcrisk_hip.h).  Not modelled: the CPA is taken on the records, not
along the chord between two of them; ``substeps`` is the refinement.  Every output is bit-identical whatever the site order, the
storm order and the launch shape.

    python -m tropical_cyclone_risk_amd.approach TRACKS.nc [TRACKS_e0.nc ...] --site=-80.1918,25.7617 --bands 50,100,200 --out approach.npz
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis, hazard, sitescan
from .analysis import DEFAULT_THRESHOLDS

PLANES = ('distance_km', 'time_h', 'v', 'speed', 'heading_deg', 'side_km', 'rmax_km')
MAX_BANDS = 8
MAX_BAND_KM = 5000.0
MAX_CELLS = sitescan.MAX_CELLS
DEFAULT_BANDS_KM = (50., 100., 200.)
BAD_BANDS = 'bands_km must be 1 to %d finite values, > 0, strictly ascending and at most %g km' % (MAX_BANDS, MAX_BAND_KM)


def hours_per_record(dt_s, substeps):
    """The unit of ``time_h``: a record's index times this is its time since the track's first sample."""
    return float(dt_s) / (3600.0 * int(substeps))


def site_closest_approach(lon, lat, v, groups, site_lon, site_lat, dt_s, bands_km=DEFAULT_BANDS_KM, thresholds=DEFAULT_THRESHOLDS,
                          rmax_km=None, substeps=1, return_planes=False, engine=None, device=0, n_groups=None):
    """The closest point of approach of every storm to every site, and passage counts by distance band and intensity.

    lon, lat, v: [n_trk][n_t] fp64 (the track file's lon_trks, lat_trks, vmax_trks).  A storm's track is its leading run of
    samples where all three are finite; a track of one sample has no records.  NumPy arrays or torch tensors on the GPU (then
    everything stays there).  dt_s: the sample spacing (s).  bands_km: 1 to 8 distances (km), finite, > 0, strictly ascending, at
    most 5000; the largest is the radius of the search.  thresholds: intensities (m/s), finite, strictly ascending;
    n_band * (n_bin + 1) <= 64.  rmax_km: None (Willoughby et al. 2006 from v and lat), a scalar, or a [n_trk][n_t] plane (km; a
    storm with a value that is not finite and > 0 on its track has no records).  substeps: 1..64 records per sample interval.
    return_planes: True, or a list of names from PLANES.  groups, n_groups, site_lon / site_lat, engine, device: as
    hazard.site_hazard.  Returns a dict: ``counts`` [n_site][n_groups][n_band][n_bin] int32, ``thresholds``, ``bands_km`` and
    ``planes``, {name: [n_site][n_trk]} of the planes asked for (NaN: no record within the largest band), in the type and on the
    device of ``lon``.
    """
    scan = _bind(groups, dt_s, bands_km, thresholds, rmax_km, substeps, n_groups)
    res, _ = scan((lon, lat, v), site_lon, site_lat, return_planes, engine, device)
    return res


def return_periods(counts, total_years):
    """[n_site][n_band][n_bin]: total_years / the passages of all groups, ``inf`` where there are none."""
    c = analysis.to_numpy(counts)
    if c.ndim != 4:
        raise ValueError('counts must be [n_site][n_groups][n_band][n_bin]')
    return hazard.return_periods(c.sum(axis=1).reshape(c.shape[0], -1), total_years).reshape(c.shape[0], c.shape[2], c.shape[3])


def wanted_planes(value):
    """The names of the planes a caller wants, in PLANES' order: all for True, none for False or None, else a list of distinct
    names from PLANES."""
    if value is True:
        return list(PLANES)
    if value is False or value is None:
        return []
    if isinstance(value, str) or not all(isinstance(k, str) for k in value) or len(set(value)) != len(list(value)):
        raise ValueError('return_planes must be True, False or a list of distinct plane names')
    if any(k not in PLANES for k in value):
        raise ValueError('return_planes names a plane that does not exist; the planes are %s' % ', '.join(PLANES))
    return [k for k in PLANES if k in value]


def _check_bands(bands_km, thresholds):
    """The approach's own argument checks (ValueError): (bands, thresholds)."""
    try:
        bands = sitescan.check_ascending(bands_km, BAD_BANDS, positive=True, max_size=MAX_BANDS)
    except TypeError:
        raise ValueError(BAD_BANDS)
    if bands[-1] > MAX_BAND_KM:
        raise ValueError(BAD_BANDS)
    thr = sitescan.check_ascending(thresholds, sitescan.ASCENDING % 'thresholds')
    if bands.size * (thr.size + 1) > MAX_CELLS:
        raise ValueError('n_band * (n_bin + 1) must be <= %d' % MAX_CELLS)
    return bands, thr


def _bind(groups, dt_s, bands_km, thresholds, rmax_km=None, substeps=1, n_groups=None):
    """site_closest_approach's arguments, checked as far as they stand alone and bound into a
    scan(tracks = (lon, lat, v), site_lon, site_lat, want, engine, device) -> (dict, Flavour): one call of tcr_approach_*, whose
    ``planes`` are those named in want (a return_planes).  The checks that need the tracks run in every call, after want's."""
    bands, thr = _check_bands(bands_km, thresholds)
    dt = sitescan.check_dt(dt_s)
    sub = sitescan.check_substeps(substeps)
    sitescan.check_n_groups(n_groups)
    rm_const = 0.0
    if rmax_km is not None and np.ndim(analysis.to_numpy(rmax_km)) == 0:
        rm_const = float(rmax_km)
        if not (np.isfinite(rm_const) and rm_const > 0):
            raise ValueError('rmax_km must be finite and > 0')
    n_band = int(bands.size)

    def scan(tracks, site_lon, site_lat, want=(), engine=None, device=0):
        want = wanted_planes(want)
        planes, fl = analysis.as_planes(tuple(tracks), 'lon, lat and v')
        if int(planes[0].shape[1]) < 1:
            raise ValueError('the tracks need at least one sample')
        if rmax_km is not None and rm_const == 0.0:
            rm_plane = fl.conv(rmax_km)
            if tuple(rm_plane.shape) != tuple(planes[0].shape):
                raise ValueError('an rmax_km plane must be [n_trk][n_t]')
            planes.append(rm_plane)
        prm = _lib.ApproachParams(dt_s=dt, substeps=sub, rmax_const_km=rm_const)

        def make_args(a, arr):
            lon_, lat_, v_ = a.planes[:3]
            rm_ = a.planes[3] if len(a.planes) > 3 else None
            n_bin_, thr_, counts_, _ = a.out
            return (C.byref(_lib.HazardTracks(lon=lon_, lat=lat_, vmax=v_, **a.tracks)), rm_, C.byref(prm)) + a.sites + \
                (n_band, bands.ctypes.data_as(_lib.DP), n_bin_, thr_, counts_, arr)
        res = sitescan.named_scan('tcr_approach', planes, fl, groups, n_groups, site_lon, site_lat, thr, n_band, PLANES, want,
                                  engine, device, make_args)
        res['bands_km'] = bands
        return res, fl
    return scan


# ---------------------------------------------------------------------------------------------------------------- CLI
def _parse_bands(text):
    try:
        return np.array([float(x) for x in text.split(',')])
    except ValueError:
        raise argparse.ArgumentTypeError('--bands: expected D1,D2,... (km), got %r' % text)


def _parse_planes(text):
    names = [k.strip() for k in text.split(',') if k.strip()]
    try:
        return wanted_planes(names)
    except ValueError as e:
        raise argparse.ArgumentTypeError('--planes: %s' % e)


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.approach',
                                description='Closest approach of every storm to sites: passages by distance band and intensity, '
                                            'their return periods, and the per-storm passage parameters.')
    analysis.add_site_args(p)
    p.add_argument('--bands', type=_parse_bands, default=np.array(DEFAULT_BANDS_KM), metavar='D1,D2,...',
                   help='1 to 8 ascending distance bands in km, at most 5000 (default: %s)' % ','.join('%g' % b for b in DEFAULT_BANDS_KM))
    analysis.add_threshold_arg(p)
    p.add_argument('--substeps', type=int, default=1, help='records per sample interval (1 = the samples only)')
    p.add_argument('--rmax-km', type=float, default=None, help='constant radius of maximum wind (default: Willoughby et al. 2006)')
    p.add_argument('--planes', type=_parse_planes, default=[], metavar='NAME,NAME,...',
                   help='also write these [n_site][n_trk] planes of the closest point of approach: ' + ', '.join(PLANES))
    analysis.add_track_args(p, 'approach.npz')
    a = analysis.finish_parse(p, p.parse_args(argv))
    try:
        _check_bands(a.bands, a.thresholds)
        sitescan.check_substeps(a.substeps)
    except ValueError as e:
        p.error(str(e))
    return a


def main(argv=None):
    args = parse_args(argv)
    inp = analysis.load_inputs(args, wind=False)
    site_lon, site_lat, total_years = inp.site_lon, inp.site_lat, inp.total_years
    scan = _bind(inp.groups, inp.dt_s, args.bands, args.thresholds, args.rmax_km, args.substeps, total_years)
    res, _ = scan((inp.lon, inp.lat, inp.vmax), site_lon, site_lat, args.planes, device=args.device)
    rp = return_periods(res['counts'], total_years)
    analysis.save_npz(args, inp, dict(counts=res['counts'], return_period=rp, bands_km=res['bands_km'], thresholds=res['thresholds'],
                                      **res['planes']), recorded=('substeps', 'rmax_km'))
    analysis.print_summary(args, inp, ', bands %s km, %d substeps' % (','.join('%g' % b for b in res['bands_km']), args.substeps))
    if site_lon.size <= 10:
        passages = res['counts'].sum(axis=1)
        analysis.print_site_tables('passages at or above (m/s) by band (rows, km): ' + ' '.join('%6g' % t for t in res['thresholds']),
                                   site_lon, site_lat, ['%6g km: ' % b for b in res['bands_km']], passages, '%6d')
        analysis.print_site_tables('return period (years) of a passage by band (rows, km) and threshold (m/s): '
                                   + ' '.join('%6g' % t for t in res['thresholds']), site_lon, site_lat,
                                   ['%6g km: ' % b for b in res['bands_km']], rp, '%6.3g')
    return 0


if __name__ == '__main__':
    sys.exit(main())
