"""Restatement in plain loops of row packing (include/tcrisk_hip.h, "row packing (event footprints)") and of the views of an event
table (tropical_cyclone_risk_amd/events.py): row_pack, by_storm, counts_from_table and dense.  Written from the header's text and the
docstrings: walk the rows and columns in order, keep what is >= the floor, append.  No value is touched by arithmetic, so
everything is compared bit for bit."""
import numpy as np


def row_pack(plane, min_value, **_):
    """(row_ptr [n_row + 1] int64, col [nnz] int32, val [nnz] fp64): the entries of every row that are >= min_value (an IEEE
    comparison: false for a NaN), in ascending column order."""
    plane = np.asarray(plane, dtype=np.float64)
    floor = np.float64(min_value)
    row_ptr, col, val = [0], [], []
    for row in plane:
        for c in range(row.shape[0]):
            if row[c] >= floor:
                col.append(c)
                val.append(row[c])
        row_ptr.append(len(col))
    return np.array(row_ptr, dtype=np.int64), np.array(col, dtype=np.int32), np.array(val, dtype=np.float64)


def by_storm(table):
    """dict(storm_ptr [n_trk + 1] int64, site [nnz] int32, value [nnz]): the entries sorted by (storm, site)."""
    ptr, storm, value, n_trk = table['site_ptr'], table['storm'], table['value'], int(table['n_trk'])
    rows = [[] for _ in range(n_trk)]
    for s in range(len(ptr) - 1):                         # sites ascend, so every storm's list comes out sorted by site
        for e in range(ptr[s], ptr[s + 1]):
            rows[storm[e]].append((s, value[e]))
    storm_ptr, site, val = [0], [], []
    for r in rows:
        site += [s for s, _ in r]
        val += [v for _, v in r]
        storm_ptr.append(len(site))
    return dict(storm_ptr=np.array(storm_ptr, dtype=np.int64), site=np.array(site, dtype=np.int32), value=np.array(val, dtype=np.float64))


def counts_from_table(table, groups, n_groups, thresholds):
    """[n_site][n_groups][n_bin] int32: the entries of a site whose storm is in group g and whose value is >= thresholds[b]."""
    ptr, storm, value = table['site_ptr'], table['storm'], table['value']
    thr = np.asarray(thresholds, dtype=np.float64)
    out = np.zeros((len(ptr) - 1, n_groups, thr.size), np.int32)
    for s in range(len(ptr) - 1):
        for e in range(ptr[s], ptr[s + 1]):
            for b in range(thr.size):
                if value[e] >= thr[b]:
                    out[s, groups[storm[e]], b] += 1
    return out


def dense(table):
    """[n_site][n_trk] fp64, NaN where the table has no entry."""
    ptr, storm, value = table['site_ptr'], table['storm'], table['value']
    out = np.full((len(ptr) - 1, int(table['n_trk'])), np.nan)
    for s in range(len(ptr) - 1):
        for e in range(ptr[s], ptr[s + 1]):
            out[s, storm[e]] = value[e]
    return out
