"""Track climatology: where storms go, form and peak, and how much power they dissipate, per cell of a lon / lat grid.

What the reference's README judges the model on (track density, genesis locations, lifetime-maximum intensity distributions,
the seasonal cycle, inter-annual count and power dissipation), computed from track files.  Per cell and per group of storms
(``csrc/tcr_climatology.hip``; the contract is in the header's "track climatology" section and DESIGN.md section 8, f-7):

- ``track``: storms with at least one live sample (lon, lat not NaN) in the cell, once per storm however often it comes back;
- ``exceed``: those whose maximum vmax over their samples in the cell is ``>= thresholds[b]``;
- ``genesis``: storms whose first live sample is in the cell; ``lmi``: storms whose lifetime maximum (the first sample attaining
  it) is in the cell;
- ``pdi``: the sum of ``q(v) = rint(v^3 * 1024)`` over the samples in the cell (``pdi / 1024 * dt`` is the power dissipation
  index in m^3 s^-2).  Integer sums: bit-identical from run to run.

Per storm: ``genesis_k``, ``lmi_v``, ``lmi_k``, ``pdi_storm``.  Samples are points: a storm can step over a cell smaller than an
hour's motion.  Host aggregates: `seasonal_cycle`, `lmi_histogram`, `annual_pdi`, `storm_counts`.

    python -m tropical_cyclone_risk_amd.climatology TRACKS.nc [...] --cells 260:350:0.25,0:60:0.25 --per-group --out clim.npz
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib, analysis
from .analysis import sample_spacing, to_numpy as _np

Q_SCALE = 1024.0                        # pdi / Q_SCALE * dt = PDI in m^3 s^-2
V_MAX = 400.0                           # vmax outside [0, V_MAX] (m/s) is rejected
MAX_SAMPLES = 1 << 27                   # n_trk * n_t: the int64 sums cannot overflow
MAX_BINS = 64
SAFFIR_SIMPSON = (33.0, 43.0, 50.0, 58.0, 70.0)     # m/s, the lower bounds of categories 1-5
MAP_FIELDS = ('track', 'exceed', 'genesis', 'lmi', 'pdi')
STORM_FIELDS = ('genesis_k', 'lmi_v', 'lmi_k', 'pdi_storm')


class CellGrid:
    """nlon x nlat cells of dlon x dlat degrees from (lon0, lat0).  A grid with nlon * dlon == 360 exactly is global: its last
    column takes what the reduction's rounding puts at 360.  Either longitude convention of the tracks lands in the same cell."""

    def __init__(self, lon0, dlon, nlon, lat0, dlat, nlat):
        self.lon0, self.dlon, self.lat0, self.dlat = (float(v) for v in (lon0, dlon, lat0, dlat))
        self.nlon, self.nlat = int(nlon), int(nlat)
        if not np.all(np.isfinite([self.lon0, self.dlon, self.lat0, self.dlat])):
            raise ValueError('the cell grid must be finite')
        if not (self.dlon > 0 and self.dlat > 0 and self.nlon >= 1 and self.nlat >= 1):
            raise ValueError('the cell grid needs dlon, dlat > 0 and nlon, nlat >= 1')
        if not self.nlon * self.dlon <= 360.0 or self.nlon * self.nlat >= 1 << 31:
            raise ValueError('the cell grid needs nlon * dlon <= 360 and nlon * nlat < 2^31')

    @classmethod
    def from_bounds(cls, lon0, lon1, lat0, lat1, d):
        """Cells of d degrees (or (dlon, dlat)) covering [lon0, lon1] x [lat0, lat1]; each span must be a whole number of cells."""
        dlon, dlat = (float(d), float(d)) if np.ndim(d) == 0 else (float(d[0]), float(d[1]))
        n = []
        for a, b, step in ((lon0, lon1, dlon), (lat0, lat1, dlat)):
            x = (float(b) - float(a)) / step if step > 0 else np.nan
            k = int(round(x)) if np.isfinite(x) else 0
            if k < 1 or abs(x - k) > 1e-9 * k:
                raise ValueError('the span %g..%g is not a whole number of %g-degree cells' % (a, b, step))
            n.append(k)
        return cls(lon0, dlon, n[0], lat0, dlat, n[1])

    @property
    def is_global(self):
        return self.nlon * self.dlon == 360.0

    @property
    def lon_edges(self):
        return self.lon0 + self.dlon * np.arange(self.nlon + 1)

    @property
    def lat_edges(self):
        return self.lat0 + self.dlat * np.arange(self.nlat + 1)

    def _c(self):
        return _lib.ClimGrid(lon0=self.lon0, dlon=self.dlon, lat0=self.lat0, dlat=self.dlat, nlon=self.nlon, nlat=self.nlat)

    def __repr__(self):
        return 'CellGrid(lon0=%r, dlon=%r, nlon=%d, lat0=%r, dlat=%r, nlat=%d)' % (self.lon0, self.dlon, self.nlon, self.lat0,
                                                                                    self.dlat, self.nlat)


def _group_index(groups, n_trk, n_groups):
    over = 'a group index is >= n_groups (or n_groups is not in [1, 2^31))'
    g, n_groups = analysis.group_index(groups, n_trk, n_groups, over=over)
    if not 1 <= n_groups < 1 << 31:
        raise ValueError(over)
    return g, n_groups


def _thresholds(thresholds):
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size > MAX_BINS or not np.all(np.isfinite(thr)) or np.any(np.diff(thr) <= 0):
        raise ValueError('thresholds: at most %d, finite and strictly ascending' % MAX_BINS)
    return thr


def track_climatology(lon, lat, vmax, groups, grid, thresholds=(), n_groups=None, engine=None, device=0):
    """Track, exceedance, genesis and LMI counts and PDI per cell of `grid` (a `CellGrid`) and group, and per storm its genesis
    sample, LMI and PDI.

    lon, lat, vmax: [n_trk][n_t] fp64 (the track file's lon_trks, lat_trks, vmax_trks; NaN past a track's end), NumPy arrays or
    torch tensors on the GPU (then everything stays there).  vmax must be NaN or in [0, 400] m/s.  groups: [n_trk] integer group
    of every storm in [0, n_groups) (default max + 1).  thresholds: at most 64, ascending (m/s).  Returns a dict of the type and
    device of ``lon``: maps ``track``, ``genesis``, ``lmi`` (int32) and ``pdi`` (int64) [n_groups][nlat][nlon], ``exceed`` (int32)
    [n_groups][n_bin][nlat][nlon]; per storm ``genesis_k``, ``lmi_k`` (int32, -1: none), ``lmi_v`` (NaN: none), ``pdi_storm``
    (int64); and ``thresholds``.  ``engine``: a TCEngine whose context is used (None: one is opened for the call).
    """
    if not isinstance(grid, CellGrid):
        grid = CellGrid(*grid)
    (lon, lat, vmax), fl = analysis.as_planes((lon, lat, vmax), 'lon, lat and vmax')
    lon, lat, vmax = (fl.contiguous(a) for a in (lon, lat, vmax))
    xp, new, ptr = fl.xp, fl.new, fl.ptr
    n_trk, n_t = int(lon.shape[0]), int(lon.shape[1])
    if n_t < 1 or n_trk * n_t > MAX_SAMPLES:
        raise ValueError('the tracks need 1 <= n_t and n_trk * n_t <= 2^27 samples')
    thr = _thresholds(thresholds)
    g, n_groups = _group_index(groups, n_trk, n_groups)
    if n_trk and bool((~xp.isnan(vmax) & ~((vmax >= 0.0) & (vmax <= V_MAX))).any()):
        raise ValueError('vmax must be NaN or in [0, %g] m/s' % V_MAX)
    n_bin, shape = int(thr.size), (n_groups, grid.nlat, grid.nlon)
    res = dict(track=new(shape, 'i4'), exceed=new((n_groups, n_bin) + shape[1:], 'i4'), genesis=new(shape, 'i4'),
               lmi=new(shape, 'i4'), pdi=new(shape, 'i8'), genesis_k=new((n_trk,), 'i4'), lmi_v=new((n_trk,), 'f8'),
               lmi_k=new((n_trk,), 'i4'), pdi_storm=new((n_trk,), 'i8'))
    gi = xp.as_tensor(g.astype(np.int32), device=fl.dev) if fl.torch else np.ascontiguousarray(g.astype(np.int32))
    out = _lib.ClimOut(**{k: (ptr(v) if k != 'exceed' or n_bin else None) for k, v in res.items()})
    trk = _lib.HazardTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=ptr(lon), lat=ptr(lat), vmax=ptr(vmax), n_group=0,
                            group_off=None)
    cg = grid._c()
    with fl.context(engine, device) as ctx:
        ctx.call('tcr_climatology', C.byref(trk), ptr(gi), n_groups, C.byref(cg), n_bin, thr.ctypes.data_as(_lib.DP), C.byref(out))
    res['thresholds'] = thr
    return res


# ---------------------------------------------------------------------------------------------------------- aggregates
def storm_counts(groups, n_groups):
    """[n_groups] storms per group (int64)."""
    g, n_groups = _group_index(groups, _np(groups).reshape(-1).shape[0], n_groups)
    return np.bincount(g, minlength=n_groups).astype(np.int64)


def annual_pdi(pdi_storm, groups, dt, n_groups):
    """[n_groups] power dissipation index per group in m^3 s^-2: the exact int64 sum of the storms' ``pdi_storm``, / 1024 * dt
    (dt: the sample spacing in s)."""
    p = _np(pdi_storm).astype(np.int64).reshape(-1)
    g, n_groups = _group_index(groups, p.size, n_groups)
    s = np.zeros(n_groups, dtype=np.int64)
    np.add.at(s, g, p)
    return s / Q_SCALE * float(dt)


def _basin_names(tc_basins):
    b = np.asarray(tc_basins)
    if b.dtype.kind == 'S':
        b = np.char.decode(b)
    return np.char.strip(b.astype(str))


def seasonal_cycle(tc_month, tc_basins, groups, n_groups, basin=None):
    """[n_groups][12] storms per genesis month (the notebook's month histogram of ``tc_month``, per group); basin: only the storms
    whose ``tc_basins`` is that basin id (the notebook's mask).  Months outside 1..12 and NaN are not counted."""
    m = np.asarray(tc_month, dtype=np.float64).reshape(-1)
    g, n_groups = _group_index(groups, m.size, n_groups)
    with np.errstate(invalid='ignore'):
        mi = np.rint(m)
        sel = (mi >= 1) & (mi <= 12)
    if basin is not None:
        sel &= _basin_names(tc_basins).reshape(-1) == str(basin)
    out = np.zeros((n_groups, 12), dtype=np.int64)
    np.add.at(out, (g[sel], mi[sel].astype(np.int64) - 1), 1)
    return out


def lmi_histogram(lmi_v, groups, bins, n_groups):
    """[n_groups][len(bins) - 1] storms per lifetime-maximum intensity bin (np.histogram's bins: [b_i, b_i+1), the last one
    closed); NaN and values outside the bins are not counted."""
    v = _np(lmi_v).astype(np.float64).reshape(-1)
    bins = np.asarray(bins, dtype=np.float64).reshape(-1)
    if bins.size < 2 or np.any(np.diff(bins) <= 0):
        raise ValueError('bins must be at least two strictly ascending edges')
    g, n_groups = _group_index(groups, v.size, n_groups)
    with np.errstate(invalid='ignore'):
        ok = (v >= bins[0]) & (v <= bins[-1])
    idx = np.minimum(np.searchsorted(bins, v[ok], side='right') - 1, bins.size - 2)
    out = np.zeros((n_groups, bins.size - 1), dtype=np.int64)
    np.add.at(out, (g[ok], idx), 1)
    return out


# ---------------------------------------------------------------------------------------------------------------- CLI
def _cells(text):
    """LON0:LON1:D,LAT0:LAT1:D"""
    try:
        lo, la = text.split(',')
        lon0, lon1, dlon = (float(x) for x in lo.split(':'))
        lat0, lat1, dlat = (float(x) for x in la.split(':'))
        return CellGrid.from_bounds(lon0, lon1, lat0, lat1, (dlon, dlat))
    except ValueError as e:
        raise argparse.ArgumentTypeError('--cells: expected LON0:LON1:D,LAT0:LAT1:D covering whole cells, got %r (%s)' % (text, e))


def _threshold_list(text):
    """LO:HI:STEP, V1,V2,... or none"""
    if text.strip().lower() == 'none':
        return np.zeros(0)
    if ':' in text:
        thr = analysis.parse_range(text, '--thresholds')
    else:
        try:
            thr = np.array([float(x) for x in text.split(',')])
        except ValueError:
            raise argparse.ArgumentTypeError('--thresholds: expected LO:HI:STEP, V1,V2,... or none, got %r' % text)
    try:
        return _thresholds(thr)
    except ValueError as e:
        raise argparse.ArgumentTypeError('--thresholds: %s' % e)


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.climatology',
                                description='Track, exceedance, genesis and LMI density, PDI, seasonal cycle and LMI distribution '
                                            'of track files.')
    p.add_argument('--cells', type=_cells, default=CellGrid.from_bounds(0.0, 360.0, -90.0, 90.0, 1.0),
                   metavar='LON0:LON1:D,LAT0:LAT1:D', help='the cell grid (default: the 1-degree globe)')
    p.add_argument('--thresholds', type=_threshold_list, default=np.array(SAFFIR_SIMPSON), metavar='LO:HI:STEP|V1,V2,..|none',
                   help='vmax thresholds of the exceedance maps in m/s (default: Saffir-Simpson categories 1-5)')
    p.add_argument('--lmi-bins', type=lambda t: analysis.parse_range(t, '--lmi-bins'), default=np.arange(0.0, 91.0, 5.0),
                   metavar='LO:HI:STEP', help='edges of the LMI histogram in m/s (default 0:90:5)')
    p.add_argument('--basin', default=None, help="seasonal cycle of the storms of this basin only (the file's tc_basins)")
    p.add_argument('--per-group', action='store_true', help='maps per (file, year) group instead of summed over groups')
    analysis.add_track_args(p, 'climatology.npz')
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    grid = args.cells
    lon, lat, vmax, groups, gfile, gyear, more = analysis.load_groups(args.tracks, extra=('tc_month', 'tc_basins', 'time'))
    n_groups = len(gfile)
    dt = sample_spacing(more['time'])
    tc_month = np.concatenate([np.asarray(m, dtype=np.float64).reshape(-1) for m in more['tc_month']])
    tc_basins = np.concatenate([_basin_names(b).reshape(-1) for b in more['tc_basins']])
    map_groups, map_n = (groups, n_groups) if args.per_group else (np.zeros(lon.shape[0], np.int64), 1)
    r = track_climatology(lon, lat, vmax, map_groups, grid, thresholds=args.thresholds, n_groups=map_n, device=args.device)
    out = {k: r[k] if args.per_group else r[k][0] for k in MAP_FIELDS}
    out.update({k: r[k] for k in STORM_FIELDS})
    series = dict(n_storms=storm_counts(groups, n_groups), annual_pdi=annual_pdi(r['pdi_storm'], groups, dt, n_groups),
                  seasonal_cycle=seasonal_cycle(tc_month, tc_basins, groups, n_groups, basin=args.basin),
                  lmi_hist=lmi_histogram(r['lmi_v'], groups, args.lmi_bins, n_groups))
    out.update(series)
    out.update(thresholds=r['thresholds'], lmi_bins=args.lmi_bins, lon_edges=grid.lon_edges, lat_edges=grid.lat_edges,
               cells=np.array([grid.lon0, grid.dlon, grid.nlon, grid.lat0, grid.dlat, grid.nlat], dtype=np.float64),
               dt=dt, q_scale=Q_SCALE, per_group=args.per_group, groups=groups, basin=str(args.basin or ''),
               **analysis.group_meta(args.tracks, gfile, gyear))
    np.savez(args.out, **out)
    n = series['n_storms']
    track = np.asarray(out['track'])
    print('%d storms, %d groups (%d files), %d x %d cells of %g x %g degrees, dt = %g s -> %s'
          % (lon.shape[0], n_groups, len(args.tracks), grid.nlon, grid.nlat, grid.dlon, grid.dlat, dt, args.out))
    print('storms per group: mean %.2f, min %d, max %d; PDI per group: mean %.4g m^3 s^-2'
          % (n.mean(), n.min(), n.max(), series['annual_pdi'].mean()))
    print('cells crossed: %d; storm-cell pairs: %d; storms with genesis in the grid: %d'
          % (int((track.reshape(-1, grid.nlat * grid.nlon).sum(axis=0) > 0).sum()), int(track.sum()), int(np.asarray(out['genesis']).sum())))
    print('seasonal cycle%s (Jan..Dec): %s' % (' of ' + args.basin if args.basin else '',
                                                ' '.join(str(int(c)) for c in series['seasonal_cycle'].sum(axis=0))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
