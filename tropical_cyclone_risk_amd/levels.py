"""Return levels: the N-year wind or rain at every site, the inverse of the per-site return periods.

With the project's formula ``return_period = total_years / count(peak >= v)`` (``hazard.return_periods``), the level of return
period ``T`` at a site is an order statistic: the ``k``-th largest storm peak there, ``k`` the smallest integer with
``k * T >= total_years`` (``loss.loss_curve``'s rule for year losses).  No thresholds and no interpolation are involved, and no
second scan: a site analysis writes its per-storm plane (``site_max``, ``site_total``, ...) for a block of sites, and one kernel
(``csrc/tcr_select.hip``) selects the ``k``-th largest value of every row that is not NaN while the block is on the device.

``row_select`` is that primitive, ``site_return_levels`` the blocked pass over any site analysis, ``ranks_of_periods`` the rule.
The contract is the header's "row selection (return levels)" section (include/tcrisk_hip.h).  ``hazard``, ``windfield`` and
``rainfall`` take ``--return-periods T1,T2,...`` on their command lines.

An order statistic stops at ``T = total_years``.  Past the record the level comes from a fitted tail: ``row_tail``
(``csrc/tcr_tail.hip``) fits a generalized Pareto distribution to the excesses of every row's ``k`` largest values over its
``(k+1)``-th by probability-weighted moments and reads the level of any return period off the fit, while the plane is on the
device; the header's "row tail fit (return levels past the record)" section is its definition.  ``site_return_levels(...,
tail_exceedances=k)`` and ``--tail-exceedances K`` add it to the blocked pass under keys of its own.
"""
import ctypes as C

import numpy as np

from . import _lib, analysis
from .sitescan import spatial_order

DEFAULT_RETURN_PERIODS = (10.0, 25.0, 50.0, 100.0, 250.0)          # (loss.DEFAULT_RETURN_PERIODS is this)
SITE_BLOCK = 64                 # sites of the scan's culling tile: a block is a multiple of it


def ranks_of_periods(return_periods, total_years):
    """(k [n_T] int64, defined [n_T] bool): the level of return period T is the k-th largest value, k the smallest integer with
    k * T >= total_years (loss.loss_curve's rule with its two rounding corrections).  ``defined`` is false for T > total_years:
    no value is exceeded that rarely, the level is NaN (k is then 1, as for T = total_years).  T finite and > 0, total_years >= 1: else ValueError."""
    total_years = int(total_years)
    if total_years < 1:
        raise ValueError('total_years must be >= 1')
    T = np.asarray(return_periods, dtype=np.float64).reshape(-1)
    if not (np.isfinite(T).all() and (T > 0).all()):
        raise ValueError('return periods must be finite and > 0')
    if (total_years / T >= 2.0 ** 62).any():
        raise ValueError('a return period is too small for total_years')
    k = np.ceil(total_years / T).astype(np.int64)
    k += (k * T < total_years)                          # the rounding of the division must not make k too small ...
    k -= ((k - 1) * T >= total_years) & (k > 1)         # ... or too large
    return k, T <= total_years


def _check_ranks(ranks):
    r = np.asarray(analysis.to_numpy(ranks))
    if r.dtype.kind not in 'iu' or r.ndim != 1 or not 1 <= r.size <= _lib.SELECT_MAX_RANKS or (r < 1).any():
        raise ValueError('ranks must be 1 to %d integers >= 1' % _lib.SELECT_MAX_RANKS)
    return np.ascontiguousarray(r.astype(np.int64))


def _row_plane(plane):
    """(Flavour, plane, n_row, n_col, row stride in values): the fp64 plane as the row kernels read it, a view whose columns are
    adjacent where it lies and anything else made contiguous first."""
    fl = analysis.Flavour(plane)
    if fl.torch:
        if plane.dtype != fl.xp.float64:
            plane = plane.to(fl.xp.float64)
    else:
        plane = np.asarray(plane, dtype=np.float64)
    if plane.ndim != 2 or int(plane.shape[1]) < 1:
        raise ValueError('plane must be [n_row][n_col] with n_col >= 1')
    n_row, n_col = int(plane.shape[0]), int(plane.shape[1])
    if fl.torch:
        s_row, s_col = (int(s) for s in plane.stride())
    else:
        s_row, s_col = (s // 8 if s % 8 == 0 else -1 for s in plane.strides)
    if not ((s_col == 1 or n_col == 1) and (s_row >= n_col or n_row <= 1)):
        plane, s_row = fl.contiguous(plane), n_col
    return fl, plane, n_row, n_col, s_row if n_row > 1 else n_col


def row_select(plane, ranks, return_valid=False, engine=None, device=0):
    """The ranks[j]-th largest value of every row of ``plane`` that is not NaN.

    plane: [n_row][n_col] fp64, a NumPy array or a torch tensor on the GPU (then the result stays there, on the current stream).
    A view whose columns are adjacent (a row stride >= n_col) is read where it lies; anything else is made contiguous first.
    ranks: 1 to 64 integers >= 1, any order, repeats allowed.  Returns ``level`` [n_row][n_rank]: one of the row's own values, bit
    for bit, in the order -inf < negatives < -0.0 < +0.0 < positives < +inf; NaN where the row holds fewer values.  With
    ``return_valid`` also ``n_valid`` [n_row] int32, the number of values of every row that are not NaN.  engine, device: as
    hazard.site_hazard."""
    ranks = _check_ranks(ranks)
    fl, plane, n_row, n_col, stride = _row_plane(plane)
    level = fl.new((n_row, ranks.size), 'f8')
    valid = fl.new((n_row,), 'i4')
    if n_row:
        with fl.context(engine, device) as ctx:
            ctx.call('tcr_select', fl.ptr(plane), n_row, n_col, stride, int(ranks.size), ranks.ctypes.data_as(C.POINTER(C.c_int64)),
                     fl.ptr(level), fl.ptr(valid))
    return (level, valid) if return_valid else level


def _check_tail(k, total_years, return_periods):
    """(k int, total_years float, T [n_T] fp64) of row_tail, or ValueError."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 2 <= int(k) <= _lib.TAIL_MAX_K:
        raise ValueError('k must be an integer in [2, %d]' % _lib.TAIL_MAX_K)
    try:
        total_years = float(total_years)
    except (TypeError, ValueError):
        raise ValueError('total_years must be finite and > 0')
    if not (np.isfinite(total_years) and total_years > 0):
        raise ValueError('total_years must be finite and > 0')
    try:
        T = np.asarray(analysis.to_numpy(return_periods), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('return periods must be finite and > 0')
    if T.ndim != 1 or not 1 <= T.size <= _lib.SELECT_MAX_RANKS or not (np.isfinite(T).all() and (T > 0).all()):
        raise ValueError('give 1 to %d return periods, finite and > 0' % _lib.SELECT_MAX_RANKS)
    return int(k), total_years, np.ascontiguousarray(T)


def row_tail(plane, k, total_years, return_periods, engine=None, device=0):
    """The levels of return periods past the record, from a generalized Pareto tail fitted to every row of ``plane``.

    plane: as row_select's.  k: the number of exceedances, an integer in [2, 2048]: per row, the k largest values that are not NaN
    are the sample and the (k+1)-th largest is the threshold.  total_years: the years the rows span (finite, > 0).
    return_periods: 1 to 64 values T, finite and > 0.  Returns a dict: ``threshold``, ``xi`` and ``sigma`` [n_row] (the threshold u,
    one of the row's own values; shape and scale by probability-weighted moments), ``level`` [n_row][n_T] (u + sigma expm1(xi L) /
    xi with L = log(k T / total_years); NaN where L < 0: T is shorter than the threshold's own return period and the order
    statistic is the answer) and ``n_valid`` [n_row] int32.  A row with fewer than k + 1 values has NaN everywhere but n_valid; a
    row whose excesses give no fit (all equal, all but one zero, an infinity) has its threshold and NaN for the rest.  The
    definition, step by step, is the header's "row tail fit (return levels past the record)" section.  engine, device: as
    row_select."""
    k, total_years, T = _check_tail(k, total_years, return_periods)
    fl, plane, n_row, n_col, stride = _row_plane(plane)
    param = fl.new((n_row, 3), 'f8')
    level = fl.new((n_row, T.size), 'f8')
    valid = fl.new((n_row,), 'i4')
    if n_row:
        with fl.context(engine, device) as ctx:
            ctx.call('tcr_tail', fl.ptr(plane), n_row, n_col, stride, k, total_years, int(T.size), T.ctypes.data_as(_lib.DP),
                     fl.ptr(param), fl.ptr(level), fl.ptr(valid))
    return dict(threshold=param[:, 0], xi=param[:, 1], sigma=param[:, 2], level=level, n_valid=valid)


TAIL_KEYS = ('tail_level', 'tail_xi', 'tail_sigma', 'tail_threshold')      # what tail_exceedances adds to site_return_levels' dict


def check_sites(site_lon, site_lat, max_bytes):
    """(Flavour, site_lon, site_lat as fp64 [n_site] of it, max_bytes) of a blocked pass, or ValueError: before any scan."""
    max_bytes = int(max_bytes)
    if max_bytes < 1:
        raise ValueError('max_bytes must be >= 1')
    fl = analysis.Flavour(site_lon)
    site_lon, site_lat = (fl.conv(a).reshape(-1) for a in (site_lon, site_lat))
    n_site = int(site_lon.shape[0])
    if int(site_lat.shape[0]) != n_site or n_site < 1:
        raise ValueError('site_lon and site_lat must be non-empty and of one length')
    if not bool(fl.xp.isfinite(site_lon).all()) or not bool(fl.xp.isfinite(site_lat).all()):
        raise ValueError('site coordinates must be finite')
    return fl, site_lon, site_lat, max_bytes


def site_blocks(scan, fl, site_lon, site_lat, key, max_bytes, n_trk=None):
    """The one block loop of the package (site_return_levels, events.site_event_table): the sites (check_sites') in spatial order
    (sitescan.spatial_order), cut into runs of max(64, max_bytes // (8 n_trk)) sites rounded down to a multiple of 64; n_trk None: a
    first block of 64 sites tells.  Yields (i, j, plane, res, order) per block: the block is the sites order[i:j], plane = res[key]
    [j - i][n_trk] is the scan's per-storm plane of it (taken out of res), res the rest of the scan's dict.  The consumer drops the
    plane before it asks for the next block."""
    n_site = int(site_lon.shape[0])
    order = spatial_order(site_lon, site_lat, fl.xp)
    slon, slat = site_lon[order], site_lat[order]
    block_of = lambda n: max(SITE_BLOCK, max_bytes // (8 * max(int(n), 1))) // SITE_BLOCK * SITE_BLOCK        # noqa: E731
    block = SITE_BLOCK if n_trk is None else block_of(n_trk)
    i = 0
    while i < n_site:
        j = min(i + block, n_site)
        res = scan(slon[i:j], slat[i:j])
        plane = res.pop(key)
        if i == 0:
            block = block_of(plane.shape[1])
        yield i, j, plane, res, order
        del plane, res
        i = j


def site_return_levels(scan, site_lon, site_lat, total_years, return_periods=DEFAULT_RETURN_PERIODS, key='site_max',
                       max_bytes=2 ** 31, n_trk=None, engine=None, device=0, tail_exceedances=None):
    """The level of every return period at every site, by a blocked pass over a site analysis.

    scan(lon_block, lat_block): any site analysis called with its per-storm plane on, returning that analysis's dict, e.g.
    ``lambda x, y: windfield.site_wind(lon, lat, v, env, groups, x, y, dt, return_max=True, n_groups=Y)``, or
    ``rainfall.site_rain(..., return_values=True)`` with ``key='site_total'``.  site_lon / site_lat: [n_site], NumPy arrays or
    torch tensors on the GPU (then the blocks, the planes and the results stay there).  The sites are put in spatial order once
    (sitescan.spatial_order) and cut into runs of max(64, max_bytes // (8 n_trk)) sites, rounded down to a multiple of 64, so that a
    block's plane res[key] [n_block][n_trk] holds about max_bytes; the plane is dropped once row_select has read it.  Returns a
    dict in the caller's site order: ``return_level`` [n_site][n_T] (NaN: fewer than k storms reach the site, or T >
    total_years), ``n_reach`` [n_site] int32 (storms with a value at the site), ``counts`` [n_site][n_groups][n_bin] as the
    unblocked call gives them, ``thresholds`` and ``return_periods``.  Every row is selected on its own and the counts of a site do
    not depend on the other sites of the call: the result does not depend on max_bytes, bit for bit.  n_trk: the number of storms
    when the caller knows it (None: a first block of 64 sites tells).  engine, device: row_select's (the scan has its own).
    tail_exceedances: None, or the k of row_tail: every block's plane then also goes through row_tail before it is dropped, and the
    dict gains ``tail_level`` [n_site][n_T] (the fitted level of every return period, also of those past total_years),
    ``tail_xi``, ``tail_sigma`` and ``tail_threshold`` [n_site], in the caller's site order; the other keys are what they are
    without it."""
    k, defined = ranks_of_periods(return_periods, total_years)
    if not 1 <= k.size <= _lib.SELECT_MAX_RANKS:
        raise ValueError('give 1 to %d return periods' % _lib.SELECT_MAX_RANKS)
    if tail_exceedances is not None:
        tail_exceedances = _check_tail(tail_exceedances, int(total_years), return_periods)[0]
    fl, site_lon, site_lat, max_bytes = check_sites(site_lon, site_lat, max_bytes)
    xp = fl.xp
    n_site = int(site_lon.shape[0])
    level = fl.new((n_site, k.size), 'f8')
    reach = fl.new((n_site,), 'i4')
    tail = None if tail_exceedances is None else (fl.new((n_site, k.size), 'f8'), fl.new((n_site, 3), 'f8'))
    counts, thr, order = None, None, None
    for i, j, plane, res, order in site_blocks(scan, fl, site_lon, site_lat, key, max_bytes, n_trk):
        if i == 0:
            thr = res['thresholds']
            counts = fl.new((n_site,) + tuple(res['counts'].shape[1:]), 'i4')
        if int(plane.shape[1]) >= 1:
            level[i:j], reach[i:j] = row_select(plane, k, return_valid=True, engine=engine, device=device)
        else:                                               # no storms at all
            level[i:j], reach[i:j] = np.nan, 0
        if tail is not None:
            if int(plane.shape[1]) >= 1:
                t = row_tail(plane, tail_exceedances, int(total_years), return_periods, engine=engine, device=device)
                tail[0][i:j] = t['level']
                tail[1][i:j, 0], tail[1][i:j, 1], tail[1][i:j, 2] = t['xi'], t['sigma'], t['threshold']
            else:
                tail[0][i:j], tail[1][i:j] = np.nan, np.nan
        counts[i:j] = res['counts']
        del plane, res

    def by_site(a):
        out = xp.empty_like(a)
        out[order] = a
        return out
    level = by_site(level)
    if not defined.all():
        level[:, xp.as_tensor(~defined, device=fl.dev) if fl.torch else ~defined] = np.nan
    res = dict(return_level=level, n_reach=by_site(reach), counts=by_site(counts), thresholds=thr,
               return_periods=np.asarray(return_periods, dtype=np.float64).reshape(-1))
    if tail is not None:
        param = by_site(tail[1])
        res.update(tail_level=by_site(tail[0]), tail_xi=param[:, 0], tail_sigma=param[:, 1], tail_threshold=param[:, 2])
    return res


# ---------------------------------------------------------------------------------------------------------------- CLI
def device_levels(analysis_fn, planes, site_lon, site_lat, total_years, return_periods, key, device, tail_exceedances=None):
    """What --return-periods does on a site analysis's command line: the track planes go to the device once as torch tensors, the
    blocked pass runs there, and site_return_levels' dict comes back as NumPy arrays.  analysis_fn(planes, lon_block, lat_block):
    the analysis with its per-storm plane on; planes: a (nested) sequence of NumPy planes, handed to it as tensors.
    tail_exceedances: what --tail-exceedances gives (site_return_levels')."""
    import torch
    dev = torch.device('cuda', int(device))

    def put(a):
        return torch.as_tensor(a, device=dev) if isinstance(a, np.ndarray) else type(a)(put(x) for x in a)
    tens = put(tuple(planes))
    # a block as large as the device has room for (the plane, and site_scan's copy of it in the caller's order): every block
    # repeats the scan's per-call work on all storms (profiles/return_levels_bench.txt: 15 blocks 2.7 x the plain call, one 1.35 x)
    max_bytes = max(2 ** 31, torch.cuda.mem_get_info(dev)[0] // 4)
    res = site_return_levels(lambda x, y: analysis_fn(tens, x, y), put(site_lon), put(site_lat), total_years, return_periods, key=key,
                             max_bytes=max_bytes, n_trk=int(planes[0].shape[0]), tail_exceedances=tail_exceedances)
    return {name: analysis.to_numpy(a) for name, a in res.items()}


def print_return_levels(res, site_lon, site_lat, unit='m/s'):
    """The return-level table of up to 10 sites (more: nothing), as analysis.print_return_periods."""
    if site_lon.size > 10:
        return
    periods = ' '.join('%6g' % t for t in res['return_periods'])
    analysis.print_site_rows('return level (%s) by return period (years): ' % unit + periods, site_lon, site_lat, res['return_level'],
                             '%6.4g')
    if 'tail_level' not in res:
        return
    rows = [' '.join('%6.4g' % v for v in res['tail_level'][i])
            + '   (xi %.3g, sigma %.4g, threshold %.4g)' % (res['tail_xi'][i], res['tail_sigma'][i], res['tail_threshold'][i])
            for i in range(site_lon.size)]
    analysis.print_site_rows('fitted tail level (%s) by return period (years): ' % unit + periods, site_lon, site_lat, rows)


def npz_keys(res):
    """What a command line adds to its .npz from site_return_levels' dict."""
    return {name: res[name] for name in ('return_level', 'return_periods', 'n_reach') + TAIL_KEYS if name in res}
