"""The Python side of the per-site scan (csrc/tcr_sitescan.h).

Eight analyses share it: site hazard, wind footprint, portfolio loss, rainfall, compound hazard, wind duration, rain
accumulation windows and directional wind.  ``site_scan`` checks the sites and groups, puts both in the order the kernel wants
(the storms of a group next to each other, the sites in Z-order), makes the call and maps every output back to the caller's site
and storm order.

The argument checks the analyses have in common live here, one function each (``check_dt``, ``check_r_out``,
``check_substeps``, ``check_n_groups``, ``check_ascending``), with the limits they test; none touches the library.

The last three analyses count several values per storm, one per row (a wind level, a window length, a compass sector), each with
an optional [n_site][n_trk] plane.  Each binds its arguments once (its ``_bind``) into a ``scan(tracks, site_lon, site_lat, want=(),
engine=None, device=0)`` -> (dict with ``planes`` = {row: plane} for the rows in want, Flavour), which its public function, its
command line and ``stacked_return_levels`` call, any number of times: every call makes its own parameter struct and keeps it, the
thresholds and the row arrays alive until the library returns.  ``wanted_rows``, ``stacked_scan``, ``stacked_planes``,
``attach_planes`` and ``stacked_return_levels`` are what they share.

A ninth analysis, the closest approach, also counts per row (a distance band), but its per-storm planes are not its rows: they are
the named parameters of the passage.  ``named_scan`` is ``stacked_scan`` for that shape."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from .analysis import group_index

# What site_scan hands an analysis's make_args, ready to pass on: ``tracks``, the fields every tracks struct has (n_trk, n_t,
# row_stride, n_group, group_off) as keywords; ``planes``, the pointers of the permuted planes; ``sites`` = (n_site, lon, lat);
# ``out`` = (n_bin, thresholds, counts, site_max); ``extras``, the pointers of the per-site extras (None stays None) and
# ``outputs``, those of the extra outputs (both empty when the analysis names none).
ScanArgs = collections.namedtuple('ScanArgs', 'tracks planes sites out extras outputs')

MAX_SUBSTEPS = 64
MAX_R_OUT_KM = 2000.0
MAX_CELLS = 64          # the cells of the scan's histogram per (site, group) (kHzMaxBin), and so the most thresholds of a call
BAD_DT = 'dt_s must be finite and > 0'
# the three wordings of check_ascending's message: % the noun, and for the footprints' thresholds in full
ASCENDING = '%s must be finite and strictly ascending'
ASCENDING_POSITIVE = '%s must be finite, > 0 and strictly ascending'
BOUNDED_THRESHOLDS = 'thresholds must be 1 to %d finite, strictly ascending values' % MAX_CELLS


# ------------------------------------------------------------------------------------------------------- shared checks
def check_dt(dt_s):
    """The sample spacing (s) as a float: finite and > 0."""
    dt_s = float(dt_s)
    if not (np.isfinite(dt_s) and dt_s > 0):
        raise ValueError(BAD_DT)
    return dt_s


def check_r_out(r_out_km):
    """The outer radius (km) as a float, in (0, MAX_R_OUT_KM]."""
    r_out_km = float(r_out_km)
    if not 0.0 < r_out_km <= MAX_R_OUT_KM:
        raise ValueError('r_out_km must be in (0, %g]' % MAX_R_OUT_KM)
    return r_out_km


def check_substeps(substeps):
    """The evaluation points per sample interval as an int, in [1, MAX_SUBSTEPS]; a bool is not an integer here."""
    if isinstance(substeps, bool) or int(substeps) != substeps or not 1 <= int(substeps) <= MAX_SUBSTEPS:
        raise ValueError('substeps must be an integer in [1, %d]' % MAX_SUBSTEPS)
    return int(substeps)


def check_n_groups(n_groups):
    """None (site_scan takes max + 1), or >= 1."""
    if n_groups is not None and int(n_groups) < 1:
        raise ValueError('n_groups must be >= 1')


def check_ascending(values, message, positive=False, max_size=None):
    """values as a contiguous fp64 vector: at least one (at most max_size), finite, strictly ascending and with positive > 0.
    message: the ValueError's text, one of the wordings above with its noun."""
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
    if a.size < 1 or (max_size is not None and a.size > max_size) or not np.isfinite(a).all() or (positive and np.any(a <= 0)) \
            or np.any(np.diff(a) <= 0):
        raise ValueError(message)
    return a


# ------------------------------------------------------------------------------------------------------------ the scan

def spatial_order(lon, lat, xp):
    """Z-order (Morton) of the sites on a 2^16 x 2^16 lon / lat raster: runs of consecutive sites are compact patches, which
    is what the kernel's per-64-site culling wants.  `xp` is numpy or torch (the same integer operations on both)."""
    to_int = (lambda a: a.astype(np.int64)) if xp is np else (lambda a: a.long())
    qx = to_int((lon % 360.0) * (65535.0 / 360.0))
    qy = to_int((lat + 90.0).clip(0.0, 180.0) * (65535.0 / 180.0))

    def spread(v):
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555
    key = spread(qx) | (spread(qy) << 1)
    return xp.argsort(key, stable=True) if xp is not np else np.argsort(key, kind='stable')


def site_scan(entry, planes, fl, groups, n_groups, site_lon, site_lat, thr, return_max, engine, device, make_args,
              site_extras=(), more_outputs=(), count_cells=None):
    """Checks the sites and groups, puts the storms of a group next to each other and the sites in spatial order, runs
    ``entry + '_dev'`` (torch tensors, on the current stream) or ``entry + '_host'`` (NumPy) and returns ``counts``,
    ``thresholds`` and with return_max ``site_max`` in the caller's site and storm order.  planes, fl: of analysis.as_planes.
    make_args(ScanArgs) -> the entry point's arguments after the context.  The library is not touched before every check here has
    passed.

    site_extras: further [n_site] inputs (or None), which go through the site permutation with the coordinates.  more_outputs:
    (name, axis) pairs of fp64 outputs along 'trk', 'group' or 'site', or 'pair' for a second [n_site][n_trk] plane like
    site_max, which come back under their names in the caller's order; an axis ('site_group', k) is an int64
    [n_site][n_groups][k] output instead.  count_cells: the counts of a (site, group) when they are
    not one per threshold (None: n_bin)."""
    xp = fl.xp
    site_lon, site_lat = (fl.conv(a).reshape(-1) for a in (site_lon, site_lat))
    if site_lon.shape[0] != site_lat.shape[0] or site_lon.shape[0] < 1:
        raise ValueError('site_lon and site_lat must be non-empty and of one length')
    if not bool(xp.isfinite(site_lon).all()) or not bool(xp.isfinite(site_lat).all()):
        raise ValueError('site coordinates must be finite')
    site_extras = [None if a is None else fl.conv(a).reshape(-1) for a in site_extras]
    if any(a is not None and a.shape[0] != site_lon.shape[0] for a in site_extras):
        raise ValueError('a per-site array must hold one value per site')
    n_trk, n_t = int(planes[0].shape[0]), int(planes[0].shape[1])
    g, n_groups = group_index(groups, n_trk, n_groups)

    # storms grouped contiguously (stable: storms keep their order inside a group), sites in spatial order
    order = np.argsort(g, kind='stable')
    group_off = np.zeros(n_groups + 1, dtype=np.int64)
    group_off[1:] = np.cumsum(np.bincount(g, minlength=n_groups))
    sorted_ = bool(np.all(order == np.arange(n_trk)))
    site_order = spatial_order(site_lon, site_lat, xp)
    n_site, n_bin = int(site_lon.shape[0]), int(thr.shape[0])
    idx = xp.as_tensor(order, device=fl.dev) if fl.torch else order
    rows = (lambda a: a.index_select(0, idx)) if fl.torch else (lambda a: a[order])
    planes = [fl.contiguous(a if sorted_ else rows(a)) for a in planes]
    if n_trk == 0:                                          # (never read, but an empty tensor has no pointer to pass)
        planes = [fl.new((1, n_t), 'f8') for _ in planes]
    slon, slat = fl.contiguous(site_lon[site_order]), fl.contiguous(site_lat[site_order])
    extras = [None if a is None else fl.contiguous(a[site_order]) for a in site_extras]
    counts = fl.new((n_site, n_groups, max(n_bin if count_cells is None else int(count_cells), 1)), 'i4')
    smax = fl.new((n_site, max(n_trk, 1)), 'f8') if return_max else None
    more = [fl.new((n_site, n_groups, int(axis[1])), 'i8') if isinstance(axis, tuple) else
            fl.new((n_site, max(n_trk, 1)) if axis == 'pair' else (max(dict(trk=n_trk, group=n_groups, site=n_site)[axis], 1),), 'f8')
            for _, axis in more_outputs]
    ptr = lambda a: None if a is None else fl.ptr(a)                                      # noqa: E731
    args = make_args(ScanArgs(
        tracks=dict(n_trk=n_trk, n_t=n_t, row_stride=n_t, n_group=n_groups, group_off=group_off.ctypes.data_as(C.POINTER(C.c_int64))),
        planes=[ptr(a) for a in planes], sites=(n_site, ptr(slon), ptr(slat)),
        out=(n_bin, thr.ctypes.data_as(_lib.DP), ptr(counts), ptr(smax)), extras=[ptr(a) for a in extras],
        outputs=[ptr(a) for a in more]))
    with fl.context(engine, device) as ctx:
        ctx.call(entry, *args)

    # back to the caller's site and storm order
    def by_site(a):
        out = xp.empty_like(a)
        out[site_order] = a
        return out
    def by_pair(a):
        out = by_site(a[:, :n_trk])
        if not sorted_:
            un = xp.empty_like(out)
            un[:, idx] = out
            out = un
        return out
    res = dict(counts=by_site(counts), thresholds=thr)
    for (name, axis), a in zip(more_outputs, more):
        if isinstance(axis, tuple):
            res[name] = by_site(a)
        elif axis == 'pair':
            res[name] = by_pair(a)
        elif axis == 'group':
            res[name] = a[:n_groups]
        elif axis == 'site':
            res[name] = by_site(a)
        else:
            res[name] = xp.empty_like(a[:n_trk])
            res[name][idx] = a[:n_trk]
    if return_max:
        res['site_max'] = by_pair(smax)
    return res


def wanted_rows(value, n_row, arg_name, row_name):
    """The sorted row indices whose planes a caller wants: all for True, none for False or None, else a list of distinct
    indices below n_row.  arg_name and row_name ('return_hours', 'level') form the two ValueError messages."""
    if value is True:
        return list(range(n_row))
    if value is False or value is None:
        return []
    try:
        want = sorted({int(i) for i in value if int(i) == i and not isinstance(i, bool)})
        if len(want) != len(list(value)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError('%s must be True, False or a list of distinct %s indices' % (arg_name, row_name))
    if any(not 0 <= i < n_row for i in want):
        raise ValueError('%s names a %s that does not exist' % (arg_name, row_name))
    return want


def stacked_scan(entry, planes, fl, groups, n_groups, site_lon, site_lat, thr, n_row, want, prefix, engine, device, make_args,
                 more_outputs=()):
    """site_scan for an entry point with n_row values per storm: ``counts`` comes back as [n_site][n_groups][n_row][n_bin] and
    ``planes`` as {row: [n_site][n_trk] plane} for the rows in want (their outputs are named prefix + row).
    make_args(ScanArgs, rows): rows is the entry point's array of n_row plane pointers (NULL for a row not wanted), or None
    when want is empty; ScanArgs.outputs holds those of more_outputs alone."""
    n_bin, n_more = int(thr.shape[0]), len(more_outputs)

    def args(a):
        rows = (C.c_void_p * n_row)()
        for i, p in zip(want, a.outputs[n_more:]):
            rows[i] = p
        return make_args(a._replace(outputs=a.outputs[:n_more]), rows if want else None)
    res = site_scan(entry, planes, fl, groups, n_groups, site_lon, site_lat, thr, False, engine, device, args,
                    more_outputs=list(more_outputs) + [('%s%d' % (prefix, i), 'pair') for i in want], count_cells=n_row * n_bin)
    n_site, n_grp = int(res['counts'].shape[0]), int(res['counts'].shape[1])
    res['counts'] = res['counts'].reshape(n_site, n_grp, n_row, n_bin)
    res['planes'] = {i: res.pop('%s%d' % (prefix, i)) for i in want}
    return res


def named_scan(entry, planes, fl, groups, n_groups, site_lon, site_lat, thr, n_row, names, want, engine, device, make_args):
    """site_scan for an entry point whose per-storm planes are not its rows (closest approach: the rows are distance bands, the
    planes the passage's parameters): ``counts`` comes back as [n_site][n_groups][n_row][n_bin] and ``planes`` as
    {name: [n_site][n_trk] plane} for the names in want (a subset of names, the entry point's fixed list of planes).
    make_args(ScanArgs, arr): arr is the entry point's array of len(names) plane pointers (NULL for a plane not wanted), or None
    when want is empty."""
    n_bin = int(thr.shape[0])
    want = [k for k in names if k in want]

    def args(a):
        arr = (C.c_void_p * len(names))()
        for k, p in zip(want, a.outputs):
            arr[names.index(k)] = p
        return make_args(a._replace(outputs=[]), arr if want else None)
    res = site_scan(entry, planes, fl, groups, n_groups, site_lon, site_lat, thr, False, engine, device, args,
                    more_outputs=[(k, 'pair') for k in want], count_cells=n_row * n_bin)
    n_site, n_grp = int(res['counts'].shape[0]), int(res['counts'].shape[1])
    res['counts'] = res['counts'].reshape(n_site, n_grp, n_row, n_bin)
    res['planes'] = {k: res.pop(k) for k in want}
    return res


def stacked_planes(fl, planes, n_row, n_site, n_trk):
    """[n_row][n_site][n_trk] from stacked_scan's ``planes``; all NaN for a row that is not among them."""
    out = fl.new((n_row, n_site, n_trk), 'f8')
    for i in range(n_row):
        out[i] = planes[i] if i in planes else np.nan
    return out


def attach_planes(res, fl, key, asked, lon):
    """The end of a stacked analysis's public function: a bound scan's ``planes`` leave its dict, and come back under key as
    stacked_planes' [n_row][n_site][n_trk] when the caller asked for any (asked: its return_* argument; lon: its first plane)."""
    planes = res.pop('planes')
    if asked is not False and asked is not None:
        n_trk = int(lon.shape[0]) if hasattr(lon, 'shape') else len(lon)
        res[key] = stacked_planes(fl, planes, int(res['counts'].shape[2]), int(res['counts'].shape[0]), n_trk)
    return res


def stacked_return_levels(scan, n_row, tracks, site_lon, site_lat, total_years, return_periods, device):
    """What --return-periods adds to the .npz of a stacked analysis: one blocked levels.device_levels pass per row, each with
    that row's plane only, and ``return_level`` stacked to [n_site][n_row][T].  scan: the analysis's bound scan, called once per
    row and site block with want = [row]; tracks: its track planes (NumPy), which go to the device once per row."""
    from . import levels

    def row_scan(i, t, x, y):
        r, _ = scan(t, x, y, want=[i])
        r['value'] = r.pop('planes')[i]
        return r
    per_row = [levels.device_levels(lambda t, x, y, i=i: row_scan(i, t, x, y), tracks, site_lon, site_lat, total_years,
                                    return_periods, 'value', device) for i in range(n_row)]
    return dict(return_level=np.stack([r['return_level'] for r in per_row], axis=1), return_periods=per_row[0]['return_periods'],
                n_reach=per_row[0]['n_reach'])
