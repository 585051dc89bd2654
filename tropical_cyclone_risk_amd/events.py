"""Event footprints: the sparse storm-by-site table of a site analysis, which storm put how much wind or rain on which site.

Every site analysis (``hazard``, ``windfield``, ``rainfall``, ...) answers a question per site, summed over storms.  The table is
the event set itself: per site, the storms whose value there is at or above a floor, with that value, as CSR.  It is the hazard
input of an external loss or vulnerability model, what a damage function of one's own is attached to, and how one asks which storms
made the 100-year wind at a site.  The dense matrix (87 001 sites x 45 000 storms x 8 B = 31 GB for the README workload, all but a
few per cent of it NaN or wind nobody cares about) exists only in blocks: a site analysis writes its per-storm plane (``site_max``,
``site_total``, ...) for a block of sites, and one device step (``csrc/tcr_rowpack.hip``) keeps, per row, the entries at or above
the floor, in column order, while the block is on the device.

``row_pack`` is that primitive, ``site_event_table`` the blocked pass over any site analysis (the block loop is
``levels.site_blocks``, shared with ``levels.site_return_levels``), ``by_storm``, ``counts_from_table`` and ``dense`` are views of a
table, ``save_events`` / ``load_events`` its file.  The contract of the device step is the header's "row packing (event
footprints)" section (include/tcrisk_hip.h).  ``hazard``, ``windfield`` and ``rainfall`` take ``--events-out FILE --events-min V`` on
their command lines.
"""
import numpy as np

from . import analysis, levels

DENSE_MAX_CELLS = 2 ** 28          # what dense() refuses to exceed: it is for small cases and tests


def _check_floor(min_value):
    """min_value as a float that is not NaN, or ValueError."""
    try:
        if isinstance(min_value, (bool, np.bool_)):
            raise TypeError
        f = float(min_value)
    except (TypeError, ValueError):
        raise ValueError('min_value must be a number that is not NaN')
    if f != f:
        raise ValueError('min_value must be a number that is not NaN')
    return f


def row_pack(plane, min_value, engine=None, device=0):
    """The entries of every row of ``plane`` that are >= ``min_value``, in column order, as CSR: ``(row_ptr, col, val)``.

    plane: [n_row][n_col] fp64, a NumPy array or a torch tensor on the GPU (then everything stays there, on the current stream,
    apart from the one read of the number of entries).  A view whose columns are adjacent (a row stride >= n_col) is read where it
    lies; anything else is made contiguous first (levels.row_select's rule).  min_value: the floor, not NaN; -inf keeps every value
    that is not NaN.  The comparison is IEEE's (a NaN is never kept, -0.0 >= 0.0 is).  Returns ``row_ptr`` [n_row + 1] int64
    (row_ptr[0] = 0, row_ptr[n_row] = nnz), ``col`` [nnz] int32 and ``val`` [nnz] fp64, the kept entries of row r in ascending column
    order from row_ptr[r] on, every value a bit copy.  The NumPy flavour crosses to the device twice, once to count and once to
    fill.  engine, device: as levels.row_select."""
    min_value = _check_floor(min_value)
    fl, plane, n_row, n_col, stride = levels._row_plane(plane)
    row_ptr = fl.new((n_row + 1,), 'i8')
    if n_row == 0:
        row_ptr[0] = 0
        return row_ptr, fl.new((0,), 'i4'), fl.new((0,), 'f8')
    with fl.context(engine, device) as ctx:
        if fl.torch:
            ctx.call('tcr_rowpack_count', fl.ptr(plane), n_row, n_col, stride, min_value, fl.ptr(row_ptr))
            nnz = int(row_ptr[n_row])                                   # the one host read of the pass
        else:
            ctx.call('tcr_rowpack', fl.ptr(plane), n_row, n_col, stride, min_value, fl.ptr(row_ptr), 0, None, None)
            nnz = int(row_ptr[n_row])
        col, val = fl.new((nnz,), 'i4'), fl.new((nnz,), 'f8')
        if nnz:
            if fl.torch:
                ctx.call('tcr_rowpack_fill', fl.ptr(plane), n_row, n_col, stride, min_value, fl.ptr(row_ptr), nnz, fl.ptr(col), fl.ptr(val))
            else:
                ctx.call('tcr_rowpack', fl.ptr(plane), n_row, n_col, stride, min_value, fl.ptr(row_ptr), nnz, fl.ptr(col), fl.ptr(val))
    return row_ptr, col, val


def _ptr_of(lengths, fl):
    """[n + 1] int64: 0, then the running sums of the lengths."""
    out = fl.new((int(lengths.shape[0]) + 1,), 'i8')
    out[0] = 0
    out[1:] = fl.xp.cumsum(lengths, 0)
    return out


def _arange(n, fl, kind='i8'):
    if fl.torch:
        return fl.xp.arange(n, dtype=fl.xp.int64 if kind == 'i8' else fl.xp.int32, device=fl.dev)
    return np.arange(n, dtype=kind)


def _cat(parts, fl, kind):
    if not parts:
        return fl.new((0,), kind)
    return fl.xp.cat(parts) if fl.torch else np.concatenate(parts)


def _row_of_entry(ptr, fl, kind='i8'):
    """[nnz]: the row of every entry of a CSR pointer."""
    n = int(ptr.shape[0]) - 1
    lengths = ptr[1:] - ptr[:-1]
    if fl.torch:
        return fl.xp.repeat_interleave(_arange(n, fl, kind), lengths)
    return np.repeat(_arange(n, fl, kind), lengths)


def site_event_table(scan, site_lon, site_lat, min_value, key='site_max', max_bytes=2 ** 31, n_trk=None, engine=None, device=0):
    """The event table of a site analysis, by a blocked pass over it: per site, the storms whose value is >= min_value.

    scan(lon_block, lat_block), site_lon / site_lat, key, max_bytes, n_trk: levels.site_return_levels' (the same contract, spatial
    order, block rule and first-block probe: both run on levels.site_blocks); every block's plane goes through row_pack and is
    dropped.  min_value: the floor, not NaN.  Returns a dict in the caller's site order: ``site_ptr`` [n_site + 1] int64, ``storm``
    [nnz] int32 (the scan's storm index: the column of the plane) and ``value`` [nnz] fp64, the entries sorted by (site, storm)
    with sites in the caller's indices; ``n_trk``, ``min_value`` and ``key``; ``counts`` [n_site][n_groups][n_bin] and
    ``thresholds`` as the unblocked call gives them.  A row is packed on its own, so the table does not depend on max_bytes, bit
    for bit.  engine, device: row_pack's (the scan has its own)."""
    min_value = _check_floor(min_value)
    fl, site_lon, site_lat, max_bytes = levels.check_sites(site_lon, site_lat, max_bytes)
    xp = fl.xp
    n_site = int(site_lon.shape[0])
    lengths = fl.new((n_site,), 'i8')                      # entries per site, in the spatial order of the blocks
    cols, vals = [], []
    counts, thr, order, n_col = None, None, None, 0
    for i, j, plane, res, order in levels.site_blocks(scan, fl, site_lon, site_lat, key, max_bytes, n_trk):
        if i == 0:
            thr = res['thresholds']
            counts = fl.new((n_site,) + tuple(res['counts'].shape[1:]), 'i4')
            n_col = int(plane.shape[1])
        if int(plane.shape[1]) >= 1:
            ptr, c, v = row_pack(plane, min_value, engine=engine, device=device)
            lengths[i:j] = ptr[1:] - ptr[:-1]
            cols.append(c)
            vals.append(v)
        else:                                               # no storms at all
            lengths[i:j] = 0
        counts[i:j] = res['counts']
        del plane, res
    # back to the caller's order: un-permute the lengths, sum them, and move every entry by the shift of its site
    col, val = _cat(cols, fl, 'i4'), _cat(vals, fl, 'f8')
    del cols, vals
    by_len = xp.empty_like(lengths)
    by_len[order] = lengths
    site_ptr, src_ptr = _ptr_of(by_len, fl), _ptr_of(lengths, fl)
    shift = site_ptr[:-1][order] - src_ptr[:-1]             # of the site at position p of the spatial order
    dst = _arange(int(col.shape[0]), fl) + shift[_row_of_entry(src_ptr, fl)]
    storm, value = xp.empty_like(col), xp.empty_like(val)
    storm[dst] = col
    value[dst] = val
    by_counts = xp.empty_like(counts)
    by_counts[order] = counts
    return dict(site_ptr=site_ptr, storm=storm, value=value, n_trk=n_col, min_value=min_value, key=key, counts=by_counts, thresholds=thr)


def by_storm(table):
    """The event-major view of a table: ``storm_ptr`` [n_trk + 1] int64, ``site`` [nnz] int32 and ``value`` [nnz], the entries sorted
    by (storm, site): a stable sort of the site-major entries by storm."""
    fl = analysis.Flavour(table['value'])
    xp, n_trk = fl.xp, int(table['n_trk'])
    site = _row_of_entry(table['site_ptr'], fl, 'i4')
    storm = table['storm']
    if fl.torch:
        perm = xp.argsort(storm, stable=True)
        per_storm = xp.bincount(storm.to(xp.int64), minlength=n_trk)
    else:
        perm = np.argsort(storm, kind='stable')
        per_storm = np.bincount(storm, minlength=n_trk).astype(np.int64)
    return dict(storm_ptr=_ptr_of(per_storm, fl), site=site[perm], value=table['value'][perm])


def counts_from_table(table, groups, n_groups, thresholds):
    """[n_site][n_groups][n_bin] int32: the entries of a site whose storm is in group g and whose value is >= thresholds[b], which is
    the ``counts`` of the scan the table came from when no threshold is below the table's floor.  groups: one non-negative integer
    per storm (analysis.group_index).  ValueError when a threshold (thresholds[0], for ascending ones) is below ``min_value``: the
    table is incomplete for that bin."""
    fl = analysis.Flavour(table['value'])
    xp, n_trk = fl.xp, int(table['n_trk'])
    thr = np.asarray(analysis.to_numpy(thresholds), dtype=np.float64).reshape(-1)
    if thr.size < 1 or not (thr >= float(table['min_value'])).all():
        raise ValueError('a threshold is below the table\'s floor (min_value): the table is incomplete for that bin')
    g, n_groups = analysis.group_index(groups, n_trk, n_groups)
    n_site = int(table['site_ptr'].shape[0]) - 1
    site = _row_of_entry(table['site_ptr'], fl)
    if fl.torch:
        g = xp.as_tensor(g, device=fl.dev)
        cell = site * n_groups + g[table['storm'].to(xp.int64)]
    else:
        cell = site * n_groups + g[table['storm']]
    out = fl.new((n_site * n_groups, thr.size), 'i4')
    for b in range(thr.size):
        n = xp.bincount(cell[table['value'] >= float(thr[b])], minlength=n_site * n_groups)
        out[:, b] = n.to(xp.int32) if fl.torch else n
    return out.reshape(n_site, n_groups, thr.size)


def dense(table):
    """[n_site][n_trk] fp64 with NaN where the table has no entry: for small cases and tests (more than 2^28 cells: ValueError)."""
    fl = analysis.Flavour(table['value'])
    n_site, n_trk = int(table['site_ptr'].shape[0]) - 1, int(table['n_trk'])
    if n_site * n_trk > DENSE_MAX_CELLS:
        raise ValueError('dense() is for small tables: %d x %d cells are more than 2^28' % (n_site, n_trk))
    out = fl.new((n_site, n_trk), 'f8')
    out[...] = np.nan
    storm = table['storm'].to(fl.xp.int64) if fl.torch else table['storm']
    out[_row_of_entry(table['site_ptr'], fl), storm] = table['value']
    return out


def save_events(path, table, site_lon, site_lat, **meta):
    """Write a table as an uncompressed .npz: ``site_ptr``, ``storm``, ``value``, ``site_lon``, ``site_lat``, ``n_trk``,
    ``min_value``, ``key`` (the table's, or meta's), ``unit`` (meta's, '' without), and whatever else ``meta`` carries, e.g. the year
    and the file index of every storm, so that a row can be traced back to a track."""
    site_lon, site_lat = (np.asarray(analysis.to_numpy(a), dtype=np.float64).reshape(-1) for a in (site_lon, site_lat))
    n_site = int(table['site_ptr'].shape[0]) - 1
    if site_lon.size != n_site or site_lat.size != n_site:
        raise ValueError('site_lon and site_lat must have the table\'s %d sites' % n_site)
    key = meta.pop('key', table.get('key', ''))
    unit = meta.pop('unit', '')
    clash = set(meta) & {'site_ptr', 'storm', 'value', 'site_lon', 'site_lat', 'n_trk', 'min_value'}
    if clash:
        raise ValueError('meta may not replace %s' % sorted(clash))
    np.savez(path, site_ptr=analysis.to_numpy(table['site_ptr']).astype(np.int64), storm=analysis.to_numpy(table['storm']).astype(np.int32),
             value=analysis.to_numpy(table['value']).astype(np.float64), site_lon=site_lon, site_lat=site_lat, n_trk=int(table['n_trk']),
             min_value=float(table['min_value']), key=str(key), unit=str(unit), **{k: analysis.to_numpy(v) for k, v in meta.items()})


def load_events(path):
    """What save_events wrote, as a dict of NumPy arrays with ``n_trk`` an int, ``min_value`` a float, ``key`` and ``unit`` strings:
    a table by_storm, counts_from_table and dense take, with the sites and the meta beside it."""
    with np.load(path) as z:
        d = {k: z[k] for k in z.files}
    d['n_trk'], d['min_value'], d['key'], d['unit'] = int(d['n_trk']), float(d['min_value']), str(d['key']), str(d['unit'])
    return d


# ---------------------------------------------------------------------------------------------------------------- CLI
def device_events(analysis_fn, planes, site_lon, site_lat, min_value, key, device):
    """What --events-out does on a site analysis's command line, as levels.device_levels: the track planes go to the device once as
    torch tensors, the blocked pass runs there, and site_event_table's dict comes back as NumPy arrays."""
    import torch
    dev = torch.device('cuda', int(device))

    def put(a):
        return torch.as_tensor(a, device=dev) if isinstance(a, np.ndarray) else type(a)(put(x) for x in a)
    tens = put(tuple(planes))
    max_bytes = max(2 ** 31, torch.cuda.mem_get_info(dev)[0] // 4)            # (levels.device_levels' block)
    res = site_event_table(lambda x, y: analysis_fn(tens, x, y), put(site_lon), put(site_lat), min_value, key=key, max_bytes=max_bytes,
                           n_trk=int(planes[0].shape[0]))
    return {name: analysis.to_numpy(a) if analysis.is_tensor(a) else a for name, a in res.items()}


def write_cli_events(args, analysis_fn, planes, site_lon, site_lat, key, unit, groups, gfile, gyear):
    """The --events-out part of a command line (a pass of its own, after the analysis): the table of analysis_fn at the floor
    --events-min, written with the year and the file index of every storm, and the largest events of up to 10 sites printed."""
    table = device_events(analysis_fn, planes, site_lon, site_lat, args.events_min, key, args.device)
    groups = np.asarray(groups, dtype=np.int64)
    storm_year, storm_file = np.asarray(gyear)[groups], np.asarray(gfile)[groups]
    save_events(args.events_out, table, site_lon, site_lat, unit=unit, storm_year=storm_year, storm_file=storm_file,
                files=np.array([str(f) for f in args.tracks]))
    print('%d events at or above %g %s at %d sites -> %s' % (table['storm'].size, args.events_min, unit, site_lon.size, args.events_out))
    print_top_events(table, site_lon, site_lat, storm_year, unit=unit)
    return table


def print_top_events(table, site_lon, site_lat, storm_year=None, unit='m/s', n_top=5):
    """The n_top largest events of up to 10 sites (more: nothing), as levels.print_return_levels: storm, year, value."""
    if site_lon.size > 10:
        return
    ptr, storm, value = (analysis.to_numpy(table[k]) for k in ('site_ptr', 'storm', 'value'))
    rows = []
    for i in range(site_lon.size):
        s, v = storm[ptr[i]:ptr[i + 1]], value[ptr[i]:ptr[i + 1]]
        top = np.argsort(-v, kind='stable')[:n_top]
        rows.append(' '.join('%d (%s) %.4g' % (s[t], '-' if storm_year is None else '%d' % storm_year[s[t]], v[t]) for t in top) or 'none')
    analysis.print_site_rows('largest events (%s) by site: storm index (year) value' % unit, site_lon, site_lat, rows)
