"""Joint site hazard: co-exceedance counts between sites, whether two sites are hit by the same storm or in the same year.

Every other site analysis treats sites one at a time.  Here a site analysis's per-storm plane (``site_max``, ``site_total``, ...)
becomes one bit per (site, level, unit) while a block of sites is on the device, a unit being a storm or a group of storms (a
year): "this unit reached this level here".  The number of units that reached a level at two sites is then the popcount of the AND
of their bit rows.  For the README grid the bits of one level are 87 001 x 704 words = 490 MB against 31 GB for the plane, and
every result is an integer.

``pack_bits`` and ``cross_counts`` are the two device steps (``csrc/tcr_joint.hip``), ``joint_hazard`` the blocked pass over any
site analysis (the block loop is ``levels.site_blocks``, shared with ``levels.site_return_levels`` and
``events.site_event_table``), ``joint_return_periods``, ``conditional`` and ``either`` read the counts.  The contract of the device
steps is the header's "joint hazard (co-exceedance between sites)" section (include/tcrisk_hip.h).

    python -m tropical_cyclone_risk_amd.joint TRACKS.nc --grid 270:300:1,10:40:1 --anchor=-80.19,25.76 --thresholds 33,50 --out joint.npz

on the wind footprint; ``--return-periods 10,50`` takes every site's own T-year wind as its level (a pass of
``levels.site_return_levels`` first), ``--unit year`` counts years instead of storms.
"""
import argparse
import sys

import numpy as np

from . import _lib, analysis, levels as levels_mod


def _check_levels(levels, n_row=None):
    """levels as a contiguous fp64 NumPy array [n_level] or [n_row][n_level] without NaN, 1 <= n_level <= 16, or ValueError."""
    try:
        lev = np.array(analysis.to_numpy(levels), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('levels must be numbers')
    if lev.ndim not in (1, 2) or not 1 <= lev.shape[-1] <= _lib.JOINT_MAX_LEVELS:
        raise ValueError('levels must be [n_level] or [n_row][n_level] with 1 <= n_level <= %d' % _lib.JOINT_MAX_LEVELS)
    if lev.ndim == 2 and n_row is not None and lev.shape[0] != n_row:
        raise ValueError('per-row levels must be [n_row][n_level]: %d rows, not %d' % (n_row, lev.shape[0]))
    if np.isnan(lev).any():
        raise ValueError('a level is NaN')
    return np.ascontiguousarray(lev)


def _check_units(unit_of, n_unit, n_col):
    """(unit_of as contiguous int32 [n_col] or None, n_unit) of pack_bits, or ValueError."""
    if unit_of is None:
        if n_unit is not None and int(n_unit) != n_col:
            raise ValueError('without unit_of, n_unit is the number of columns')
        return None, n_col
    u = np.asarray(analysis.to_numpy(unit_of))
    if u.ndim != 1 or u.shape[0] != n_col or u.dtype.kind not in 'iu':
        raise ValueError('unit_of must hold one integer per column')
    n_unit = int(n_unit if n_unit is not None else u.max() + 1)
    if not 1 <= n_unit <= _lib.JOINT_MAX_MAPPED_UNITS:
        raise ValueError('with unit_of, n_unit must be in [1, %d]' % _lib.JOINT_MAX_MAPPED_UNITS)
    if u.min() < 0 or u.max() >= n_unit:
        raise ValueError('an entry of unit_of is not in [0, n_unit)')
    return np.ascontiguousarray(u.astype(np.int32)), n_unit


def _on_device(fl, device):
    """(torch, the device of a call): the tensors' own, or for the NumPy flavour the device index given."""
    import torch
    return torch, (fl.dev if fl.torch else torch.device('cuda', int(device)))


def pack_bits(plane, levels, unit_of=None, n_unit=None, engine=None, device=0):
    """One bit per (level, row, unit) of ``plane``: ``(bits [n_level][n_row][n_word], n_set [n_level][n_row] int32)``.

    plane: [n_row][n_col] fp64, a NumPy array or a torch tensor on the GPU (then the result stays there, on the current stream), read
    where it lies when its columns are adjacent (levels.row_select's rule).  levels: [n_level], the same for every row, or
    [n_row][n_level]; 1 to 16 per row, not NaN.  Column c of row r reaches level l iff plane[r][c] >= levels[r][l] as an IEEE
    comparison (a NaN never does, -0.0 >= 0.0 does, -inf admits every value that is not NaN).  unit_of None: unit = column, n_unit
    = n_col.  Otherwise unit_of [n_col] integers in [0, n_unit) (n_unit None: max + 1; at most 2^18), and bit u is set iff any column
    of unit u reaches the level; units may be empty and in any order.  Bit u & 63 of word u >> 6 is unit u, n_word = ceil(n_unit /
    64), the bits past n_unit are zero; n_set is the popcount of a row.  Bits are uint64 in NumPy and int64 with the same bit pattern
    in torch.  The NumPy flavour goes through tensors on ``device``.  engine, device: as levels.row_select."""
    fl, plane, n_row, n_col, stride = levels_mod._row_plane(plane)
    lev = _check_levels(levels, n_row)
    unit_of, n_unit = _check_units(unit_of, n_unit, n_col)
    n_level, n_word = int(lev.shape[-1]), (n_unit + 63) // 64
    if lev.ndim == 1:
        lev = np.repeat(lev[None, :], n_row, axis=0)                       # (one row per row of the plane)
    if n_row == 0:
        if fl.torch:
            return fl.new((n_level, 0, n_word), 'i8'), fl.new((n_level, 0), 'i4')
        return np.empty((n_level, 0, n_word), np.uint64), np.empty((n_level, 0), np.int32)
    _lib.lib()                                              # (the library, before anything goes to the device)
    torch, dev = _on_device(fl, device)
    if not fl.torch:
        plane, stride = torch.as_tensor(np.ascontiguousarray(plane), device=dev), n_col
    t_lev = torch.as_tensor(lev, device=dev)
    t_unit = None if unit_of is None else torch.as_tensor(unit_of, device=dev)
    bits = torch.empty((n_level, n_row, n_word), dtype=torch.int64, device=dev)
    n_set = torch.empty((n_level, n_row), dtype=torch.int32, device=dev)
    with analysis.Context(engine, dev) as ctx:
        ctx.call('tcr_joint_pack', plane.data_ptr(), n_row, n_col, stride, t_lev.data_ptr(), n_level,
                 None if t_unit is None else t_unit.data_ptr(), n_unit, bits.data_ptr(), n_row * n_word, n_set.data_ptr(), n_row)
    if fl.torch:
        return bits, n_set
    return bits.cpu().numpy().view(np.uint64), n_set.cpu().numpy()


def _check_bits(bits, what):
    """A bit table as [n_level][n_row][n_word] of 64-bit integers, or ValueError."""
    if analysis.is_tensor(bits):
        import torch
        ok = bits.dtype == torch.int64
    else:
        bits = np.asarray(bits)
        ok = bits.dtype in (np.dtype(np.uint64), np.dtype(np.int64))
    if not ok or bits.ndim != 3 or not 1 <= int(bits.shape[0]) <= _lib.JOINT_MAX_LEVELS:
        raise ValueError('%s must be [n_level][n_row][n_word] 64-bit integers with 1 <= n_level <= %d' % (what, _lib.JOINT_MAX_LEVELS))
    return bits


def cross_counts(bits_a, bits_b=None, engine=None, device=0):
    """[n_level][n_a][n_b] int32: counts[l][i][j] = the number of bits set in both bits_a[l][i] and bits_b[l][j].

    bits_a, bits_b: tables of pack_bits with the same levels and words (bits_b None: bits_a with itself), NumPy arrays or torch
    tensors on the GPU (then the counts stay there, on the current stream); the NumPy flavour goes through tensors on ``device``.
    A table whose rows are contiguous is read where it lies (a block of rows of a larger table is); anything else is copied."""
    bits_a = _check_bits(bits_a, 'bits_a')
    bits_b = bits_a if bits_b is None else _check_bits(bits_b, 'bits_b')
    if analysis.is_tensor(bits_a) != analysis.is_tensor(bits_b):
        raise ValueError('bits_a and bits_b must both be NumPy arrays or both tensors')
    if tuple(bits_a.shape[::2]) != tuple(bits_b.shape[::2]):
        raise ValueError('bits_a and bits_b must have the same levels and words')
    fl = analysis.Flavour(bits_a)
    n_level, n_a, n_word = (int(s) for s in bits_a.shape)
    n_b = int(bits_b.shape[1])
    if n_a == 0 or n_b == 0 or n_word == 0:
        out = fl.new((n_level, n_a, n_b), 'i4')
        out[...] = 0
        return out
    _lib.lib()
    torch, dev = _on_device(fl, device)

    def table(t):
        if not fl.torch:
            t = torch.as_tensor(np.ascontiguousarray(t).view(np.int64), device=dev)
        s = tuple(int(x) for x in t.stride())
        if not (s[2] == 1 or n_word == 1) or not (s[1] == n_word or int(t.shape[1]) == 1) or (n_level > 1 and s[0] < int(t.shape[1]) * n_word):
            t = t.contiguous()
            s = tuple(int(x) for x in t.stride())
        return t, (s[0] if n_level > 1 else int(t.shape[1]) * n_word)
    same = bits_b is bits_a
    ta, sa = table(bits_a)
    tb, sb = (ta, sa) if same else table(bits_b)
    counts = torch.empty((n_level, n_a, n_b), dtype=torch.int32, device=dev)
    with analysis.Context(engine, dev) as ctx:
        ctx.call('tcr_joint_cross', ta.data_ptr(), n_a, sa, tb.data_ptr(), n_b, sb, n_word, n_level, counts.data_ptr())
    return counts if fl.torch else counts.cpu().numpy()


def _check_anchors(anchors, n_site):
    """anchors as int64 site indices [n_a] (None: every site), or ValueError."""
    if anchors is None:
        return np.arange(n_site, dtype=np.int64)
    a = np.asarray(analysis.to_numpy(anchors))
    if a.ndim != 1 or a.size < 1 or a.dtype.kind not in 'iu' or a.min() < 0 or a.max() >= n_site:
        raise ValueError('anchors must be site indices in [0, n_site)')
    return a.astype(np.int64)


def joint_hazard(scan, site_lon, site_lat, levels, anchors=None, key='site_max', unit='storm', groups=None, n_groups=None,
                 max_bytes=2 ** 31, max_out_bytes=2 ** 31, n_trk=None, engine=None, device=0):
    """The co-exceedance counts between sites of a site analysis, by a blocked pass over it.

    scan(lon_block, lat_block), site_lon / site_lat, key, max_bytes, n_trk: levels.site_return_levels' (the same contract, spatial
    order, block rule and first-block probe: all three run on levels.site_blocks); every block's plane goes through pack_bits into
    one bit table and is dropped, then cross_counts crosses the rows of the anchors with all sites.  levels: [n_level] absolute
    levels, or [n_site][n_level] per site in the caller's order (e.g. every site's own return levels); 1 to 16, not NaN.  anchors:
    site indices (None: every site).  unit: 'storm' (a unit is a storm: "hit by the same storm") or 'group' (a unit is a group of
    storms, groups / n_groups as analysis.group_index takes them: "hit in the same year"; at most 2^18 groups).  max_out_bytes: what
    ``joint`` may take; more raises ValueError ("choose anchors") before any scan.  Returns a dict in the caller's site order:
    ``joint`` [n_level][n_a][n_site] int32 (units that reached level l at anchor a and at site j), ``n_set`` [n_level][n_site] int32
    (units that reached it at site j: joint of a site with itself), ``anchors``, ``levels``, ``n_unit``, and ``counts``
    [n_site][n_groups][n_bin] and ``thresholds`` as the unblocked scan gives them.  A row is packed on its own and a count is a
    sum of integers: the result does not depend on max_bytes, bit for bit.  engine, device: pack_bits' (the scan has its own)."""
    fl, site_lon, site_lat, max_bytes = levels_mod.check_sites(site_lon, site_lat, max_bytes)
    xp = fl.xp
    n_site = int(site_lon.shape[0])
    lev = _check_levels(levels, n_site)
    n_level = int(lev.shape[-1])
    all_pairs = anchors is None
    anchors = _check_anchors(anchors, n_site)
    if unit not in ('storm', 'group'):
        raise ValueError('unit must be \'storm\' or \'group\'')
    unit_of, n_unit = None, None
    if unit == 'group':
        if groups is None:
            raise ValueError('unit=\'group\' needs groups')
        n_g = int(np.asarray(analysis.to_numpy(groups)).reshape(-1).shape[0])
        if n_trk is not None and int(n_trk) != n_g:
            raise ValueError('groups must hold one non-negative integer per storm')
        g, n_unit = analysis.group_index(groups, n_g, n_groups)
        if not 1 <= n_unit <= _lib.JOINT_MAX_MAPPED_UNITS:
            raise ValueError('unit=\'group\' takes 1 to %d groups' % _lib.JOINT_MAX_MAPPED_UNITS)
        unit_of = g.astype(np.int32)
    if n_level * anchors.size * n_site * 4 > int(max_out_bytes):
        raise ValueError('joint [%d][%d][%d] int32 is more than max_out_bytes = %d: choose anchors' % (n_level, anchors.size, n_site,
                                                                                                       int(max_out_bytes)))

    def to_fl(a, kind):
        return xp.as_tensor(a, device=fl.dev) if fl.torch else np.asarray(a, dtype=kind)
    table, n_set, counts, thr, order, lev_sp = None, None, None, None, None, lev
    for i, j, plane, res, order in levels_mod.site_blocks(scan, fl, site_lon, site_lat, key, max_bytes, n_trk):
        if i == 0:
            thr = res['thresholds']
            counts = fl.new((n_site,) + tuple(res['counts'].shape[1:]), 'i4')
            n_col = int(plane.shape[1])
            if unit_of is not None and unit_of.shape[0] != n_col:
                raise ValueError('groups must hold one non-negative integer per storm: %d storms, not %d' % (n_col, unit_of.shape[0]))
            if unit_of is None:
                n_unit = n_col
            n_word = (n_unit + 63) // 64
            table = fl.new((n_level, n_site, n_word), 'i8') if fl.torch else np.empty((n_level, n_site, n_word), np.uint64)
            n_set = fl.new((n_level, n_site), 'i4')
            if lev.ndim == 2:
                lev_sp = lev[analysis.to_numpy(order)]           # per-site levels, in the spatial order of the blocks
        if int(plane.shape[1]) >= 1:
            b, n = pack_bits(plane, lev_sp if lev.ndim == 1 else lev_sp[i:j], unit_of=unit_of, n_unit=n_unit, engine=engine, device=device)
            table[:, i:j], n_set[:, i:j] = b, n
        else:                                               # no storms at all
            table[:, i:j], n_set[:, i:j] = 0, 0
        counts[i:j] = res['counts']
        del plane, res
    # the table stays in spatial order: the anchors' rows are looked up there (all pairs: the table with itself), and the rows and
    # columns of the counts go back to the caller's order
    inv = np.empty(n_site, np.int64)
    inv[analysis.to_numpy(order)] = np.arange(n_site)
    if int(table.shape[2]) == 0:
        joint_sp = fl.new((n_level, anchors.size, n_site), 'i4')
        joint_sp[...] = 0
    elif all_pairs:
        joint_sp = cross_counts(table, engine=engine, device=device)
    else:
        joint_sp = cross_counts(table[:, to_fl(inv[anchors], 'i8')], table, engine=engine, device=device)
    joint, set_site, by_counts = xp.empty_like(joint_sp), xp.empty_like(n_set), xp.empty_like(counts)
    if all_pairs:
        joint[:, order[:, None], order[None, :]] = joint_sp
    else:
        joint[:, :, order] = joint_sp
    set_site[:, order] = n_set
    by_counts[order] = counts
    return dict(joint=joint, n_set=set_site, anchors=anchors, levels=lev, n_unit=int(n_unit), counts=by_counts, thresholds=thr)


# ------------------------------------------------------------------------------------------------------- reading counts
def _float(a, fl):
    return a.to(fl.xp.float64) if fl.torch else np.asarray(a, dtype=np.float64)


def _anchor_set(n_set, anchors, fl):
    """[n_level][n_a][1]: n_set of the anchors."""
    a = fl.xp.as_tensor(analysis.to_numpy(anchors).astype(np.int64), device=fl.dev) if fl.torch else np.asarray(anchors, dtype=np.int64)
    return n_set[:, a][:, :, None]


def joint_return_periods(joint, total_years):
    """total_years / joint, ``inf`` where the count is 0 (hazard.return_periods' rule), in the flavour of ``joint``: with unit='group'
    and one group per year the return period of both sites reaching the level in one season, with unit='storm' in one event."""
    fl = analysis.Flavour(joint)
    c = _float(joint, fl)
    one, inf = fl.xp.ones_like(c), fl.xp.full_like(c, np.inf)
    return fl.xp.where(c > 0, float(total_years) / fl.xp.where(c > 0, c, one), inf)


def conditional(joint, n_set, anchors):
    """P(site reaches | anchor reaches) = joint[l][a][j] / n_set[l][anchors[a]], NaN where the anchor never reaches the level."""
    fl = analysis.Flavour(joint)
    c, n = _float(joint, fl), _float(_anchor_set(n_set, anchors, fl), fl)
    one, nan = fl.xp.ones_like(n), fl.xp.full_like(c, np.nan)
    return fl.xp.where(n > 0, c / fl.xp.where(n > 0, n, one), nan)


def either(joint, n_set, anchors):
    """Units in which the anchor or the site reaches the level: n_set[l][anchors[a]] + n_set[l][j] - joint[l][a][j]."""
    fl = analysis.Flavour(joint)
    return _anchor_set(n_set, anchors, fl) + n_set[:, None, :] - joint


# ---------------------------------------------------------------------------------------------------------------- CLI
def parse_levels(text):
    try:
        v = [float(x) for x in text.split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError('--thresholds: expected V1,V2,..., got %r' % text)
    if not 1 <= len(v) <= _lib.JOINT_MAX_LEVELS or any(x != x for x in v):
        raise argparse.ArgumentTypeError('--thresholds: need 1 to %d values that are not NaN, got %r' % (_lib.JOINT_MAX_LEVELS, text))
    return np.array(v)


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tropical_cyclone_risk_amd.joint',
                                description='Co-exceedance counts of the wind footprint between sites: hit by the same storm, or in the same year.')
    analysis.add_site_args(p)
    p.add_argument('--sites-csv', dest='sites', metavar='FILE.csv', help='the same as --sites')
    p.add_argument('--anchor', type=analysis.parse_site, action='append', default=[], metavar='LON,LAT',
                   help='repeatable: the sites every site is paired with (added to the sites when not among them); none: all pairs')
    analysis.add_footprint_args(p)
    p.add_argument('--thresholds', type=parse_levels, default=None, metavar='V1,V2,...', help='absolute levels (m/s)')
    p.add_argument('--return-periods', type=analysis.parse_periods, default=None, metavar='T1,T2,...',
                   help='every site\'s own T-year peak wind as its levels (levels.site_return_levels: a pass of its own)')
    p.add_argument('--unit', choices=('storm', 'year'), default='storm', help='what is counted: storms, or years (the files\' groups)')
    analysis.add_track_args(p, 'joint.npz')
    a = p.parse_args(argv)
    if (a.thresholds is None) == (a.return_periods is None):
        p.error('give exactly one of --thresholds and --return-periods')
    if a.return_periods is not None and a.return_periods.size > _lib.JOINT_MAX_LEVELS:
        p.error('--return-periods: at most %d' % _lib.JOINT_MAX_LEVELS)
    return analysis.finish_parse(p, a)


def cli_sites(args):
    """(site_lon, site_lat, anchors): the sites of the command line with every --anchor among them (appended when it is not), and
    the anchors' indices (None without --anchor)."""
    lon, lat = analysis.collect_sites(args)
    lon, lat, idx = list(lon), list(lat), []
    for x, y in args.anchor:
        hit = [k for k in range(len(lon)) if lon[k] == x and lat[k] == y]
        if not hit:
            lon.append(x)
            lat.append(y)
            hit = [len(lon) - 1]
        idx.append(hit[0])
    return np.array(lon, dtype=np.float64), np.array(lat, dtype=np.float64), (np.array(idx, dtype=np.int64) if idx else None)


def main(argv=None):
    import torch
    from . import windfield
    args = parse_args(argv)
    site_lon, site_lat, anchors = cli_sites(args)
    inp = analysis.load_inputs(args, wind=True, sites=(site_lon, site_lat))
    kw = dict(rmax_km=args.rmax_km, ck_cd=args.ck_cd, r_out_km=args.r_out_km, substeps=args.substeps, n_groups=inp.total_years)
    planes = (inp.lon, inp.lat, inp.v, tuple(inp.env))

    def block(t, x, y):
        return windfield.site_wind(t[0], t[1], t[2], t[3], inp.groups, x, y, inp.dt_s, return_max=True, **kw)
    more = {}
    if args.return_periods is not None:
        rl = levels_mod.device_levels(block, planes, site_lon, site_lat, inp.total_years, args.return_periods, 'site_max', args.device)
        lev = np.where(np.isnan(rl['return_level']), np.inf, rl['return_level'])
        n_never = int(np.isnan(rl['return_level']).any(axis=1).sum())
        print('%d of %d sites have no level for a return period (fewer storms reach them): they never exceed it' % (n_never, site_lon.size))
        more = dict(return_periods=rl['return_periods'], return_level=rl['return_level'])
    else:
        lev = args.thresholds
    dev = torch.device('cuda', int(args.device))

    def put(a):
        return torch.as_tensor(a, device=dev) if isinstance(a, np.ndarray) else type(a)(put(x) for x in a)
    tens = put(planes)
    max_bytes = max(2 ** 31, torch.cuda.mem_get_info(dev)[0] // 4)            # (levels.device_levels' block)
    res = joint_hazard(lambda x, y: block(tens, x, y), put(site_lon), put(site_lat), lev, anchors=anchors, unit='group' if args.unit == 'year' else 'storm',
                       groups=inp.groups, n_groups=inp.total_years, max_bytes=max_bytes, n_trk=int(inp.lon.shape[0]))
    res = {k: analysis.to_numpy(v) if analysis.is_tensor(v) else v for k, v in res.items()}
    rp = joint_return_periods(res['joint'], inp.total_years)
    cond = conditional(res['joint'], res['n_set'], res['anchors'])
    analysis.save_npz(args, inp, dict(joint=res['joint'], n_set=res['n_set'], anchors=res['anchors'], levels=res['levels'], n_unit=res['n_unit'],
                                      unit=args.unit, joint_return_period=rp, conditional=cond, counts=res['counts'], thresholds=res['thresholds']),
                      recorded=('r_out_km', 'substeps', 'rmax_km'), more=more)
    analysis.print_summary(args, inp, ', %d anchors, %d levels, %d %ss' % (res['anchors'].size, res['joint'].shape[0], res['n_unit'], args.unit))
    what = ('level %g m/s' % v for v in lev) if args.return_periods is None else ('own %g-year level' % t for t in args.return_periods)
    for l, name in enumerate(what):
        for a in res['anchors'][:10]:
            k = int(np.nonzero(res['anchors'] == a)[0][0])
            print('anchor (%.4f, %.4f), %s: %d %ss reach it there' % (site_lon[a], site_lat[a], name, res['n_set'][l, a], args.unit))
            rows = ['joint %6d   return period %8.4g   P(site | anchor) %6.3g' % (res['joint'][l, k, j], rp[l, k, j], cond[l, k, j])
                    for j in range(min(site_lon.size, 10))]
            analysis.print_site_rows(None, site_lon[:10], site_lat[:10], rows)
    return 0


if __name__ == '__main__':
    sys.exit(main())
