"""Event footprints (tropical_cyclone_risk_amd/events.py, csrc/tcr_rowpack.hip): the entries of every row of a per-storm plane at or
above a floor as CSR, and the blocked pass that turns a site analysis into the sparse storm-by-site table.  CPU tests pin the
restatement in plain loops (tests/events_numpy.py) to hand values and check the argument handling, the blocked driver on a scan
made of NumPy, the views and the file; GPU tests (`-m gpu`) check the kernels against the restatement through both entry points, and
the table against the plane and the counts of the scan it comes from.  Nothing here has a tolerance: every comparison is of bits,
NaN equal to NaN."""
import ctypes
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import events_numpy as EN
from tests.levels_numpy import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_NAN = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]        # a NaN with the sign bit set (and a payload)
#                       0    1     2       3       4        5    6     7        8       9        10    11
SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3.5, -3.5, NEG_NAN, 1e-310, -1e-310, 17.5, 17.5])
SPECIAL_KEPT = ((0.0, [0, 1, 3, 5, 8, 10, 11]), (-0.0, [0, 1, 3, 5, 8, 10, 11]), (-np.inf, [0, 1, 3, 4, 5, 6, 8, 9, 10, 11]),
                (np.inf, [3]), (17.5, [3, 10, 11]), (3.5, [3, 5, 10, 11]))


def _same_csr(got, want):
    """(row_ptr, col, val) against (row_ptr, col, val): integers equal, values the same bits."""
    return (got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float64 and np.array_equal(got[0], want[0])
            and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2]))


def _same_table(a, b):
    return (np.array_equal(a['site_ptr'], b['site_ptr']) and np.array_equal(a['storm'], b['storm']) and same_bits(a['value'], b['value'])
            and np.array_equal(a['counts'], b['counts']) and np.array_equal(a['thresholds'], b['thresholds'])
            and a['n_trk'] == b['n_trk'] and a['min_value'] == b['min_value'])


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_by_hand():
    assert np.isnan(NEG_NAN) and np.signbit(NEG_NAN)
    for floor, cols in SPECIAL_KEPT:
        ptr, col, val = EN.row_pack(SPECIAL[None, :], floor)
        assert ptr.tolist() == [0, len(cols)] and col.tolist() == cols, floor
        assert _same_csr((ptr, col, val), (ptr, np.array(cols, np.int32), SPECIAL[cols]))
    ptr, col, val = EN.row_pack(SPECIAL[None, :], 0.0)
    assert not np.signbit(val[0]) and np.signbit(val[1]) and val[4] == 1e-310            # a kept -0.0 stays -0.0; the subnormal
    # an empty row, a row kept whole, and a row between them
    plane = np.array([[np.nan, NEG_NAN, 1.0, 2.0], [5.0, 2.5, np.inf, 9.0], [2.5, 0.0, 2.4999, 3.0]])
    ptr, col, val = EN.row_pack(plane, 2.5)
    assert ptr.tolist() == [0, 0, 4, 6] and col.tolist() == [0, 1, 2, 3, 0, 3] and same_bits(val, [5.0, 2.5, np.inf, 9.0, 2.5, 3.0])
    assert ptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float64
    ptr, col, val = EN.row_pack(np.zeros((0, 4)), 0.0)
    assert ptr.tolist() == [0] and col.size == 0 and val.size == 0
    # the views, on a table of three sites and four storms written by hand
    table = dict(site_ptr=np.array([0, 2, 2, 5]), storm=np.array([1, 3, 0, 1, 2], np.int32), value=np.array([20.0, 30.0, 12.0, 40.0, 10.0]),
                 n_trk=4, min_value=10.0)
    ev = EN.by_storm(table)
    assert ev['storm_ptr'].tolist() == [0, 1, 3, 4, 5] and ev['site'].tolist() == [2, 0, 2, 2, 0] and ev['value'].tolist() == [12.0, 20.0, 40.0, 10.0, 30.0]
    d = EN.dense(table)
    assert same_bits(d, [[np.nan, 20.0, np.nan, 30.0], [np.nan] * 4, [12.0, 40.0, 10.0, np.nan]])
    c = EN.counts_from_table(table, np.array([0, 1, 1, 0]), 2, [10.0, 25.0])
    assert c.tolist() == [[[1, 1], [1, 0]], [[0, 0], [0, 0]], [[1, 0], [2, 1]]]


def test_rowpack_symbols_exported_constant_and_abi_version_unchanged(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_rowpack_count_dev', 'tcr_rowpack_fill_dev', 'tcr_rowpack_host'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    L.tcr_abi_version.restype = ctypes.c_int
    assert L.tcr_abi_version() == 7 and _lib.TCR_ABI_VERSION == 7
    src = '#include <stdio.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%d\\n",TCR_ROWPACK_UNROLL);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'k.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'k')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        assert int(subprocess.check_output([exe])) == _lib.ROWPACK_UNROLL
    assert _lib.ROWPACK_UNROLL >= 1


def test_argument_errors_before_any_device_work(monkeypatch):
    from tropical_cyclone_risk_amd import _lib, events

    def no_library():
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', no_library)
    plane = np.arange(12.0).reshape(3, 4)
    for floor in (np.nan, NEG_NAN, 'x', None, True):
        with pytest.raises(ValueError):
            events.row_pack(plane, floor)
    for bad in (np.arange(4.0), np.zeros((3, 0)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            events.row_pack(bad, 1.0)
    ptr, col, val = events.row_pack(np.zeros((0, 4)), 1.0)                # no rows: nothing to ask the library
    assert ptr.tolist() == [0] and ptr.dtype == np.int64 and col.dtype == np.int32 and col.size == 0 and val.size == 0
    with pytest.raises(AssertionError, match='the library was touched'):
        events.row_pack(plane, 1.0)

    def scan(x, y):
        raise AssertionError('the scan was called before the arguments were checked')
    lon, lat = np.array([280.0, 281.0]), np.array([20.0, 21.0])
    for kw in (dict(min_value=np.nan), dict(min_value='x'), dict(max_bytes=0), dict(site_lat=lat[:1]), dict(site_lat=np.array([np.nan, 1.0])),
               dict(site_lon=np.array([np.inf, 1.0])), dict(site_lon=np.array([]), site_lat=np.array([]))):
        with pytest.raises(ValueError):
            events.site_event_table(**dict(dict(scan=scan, site_lon=lon, site_lat=lat, min_value=10.0), **kw))
    with pytest.raises(AssertionError, match='the scan was called'):
        events.site_event_table(scan, lon, lat, 10.0)


def _fake_scan(rng, n_trk=37, n_groups=4):
    """A site analysis made of NumPy (the idea of test_levels._fake_scan): storm s is a disc of radius r_s degrees around (cx_s,
    cy_s) with peak p_s, and a site's value of it falls off with the distance (NaN outside).  A site's row depends on that site
    alone, as in the real scans.  Storm 5 peaks at exactly 10.0, the first threshold; storm 7 stays below it everywhere."""
    cx, cy, rad, peak = rng.uniform(270, 300, n_trk), rng.uniform(10, 40, n_trk), rng.uniform(2, 12, n_trk), rng.uniform(15, 80, n_trk)
    peak[5], peak[7] = 10.0, 5.0
    groups = rng.integers(0, n_groups, n_trk)
    thr = np.array([10.0, 20.0, 30.0, 50.0])
    calls = []

    def plane(x, y):
        d = np.hypot(x[:, None] - cx[None, :], y[:, None] - cy[None, :])
        return np.where(d <= rad[None, :], peak[None, :] * (1.0 - 0.08 * d), np.nan)

    def scan(x, y):
        calls.append((np.array(x), np.array(y)))
        m = plane(np.asarray(x), np.asarray(y))
        counts = np.zeros((m.shape[0], n_groups, thr.size), np.int32)
        for g in range(n_groups):
            counts[:, g] = (m[:, groups == g, None] >= thr[None, None, :]).sum(axis=1)
        return dict(counts=counts, thresholds=thr, site_max=m)
    return scan, plane, calls, thr, groups, (cx, cy)


def test_blocked_driver_equals_the_unblocked_plane_in_the_callers_site_order(monkeypatch):
    from tropical_cyclone_risk_amd import events
    from tropical_cyclone_risk_amd.sitescan import spatial_order
    monkeypatch.setattr(events, 'row_pack', EN.row_pack)
    rng = np.random.default_rng(11)
    scan, plane, calls, thr, groups, (cx, cy) = _fake_scan(rng)
    slon, slat = rng.uniform(268, 302, 130), rng.uniform(8, 42, 130)
    slon[17], slat[17] = 100.0, -30.0                                  # no storm reaches this one
    slon[40], slat[40] = cx[5], cy[5]                                  # the eye of storm 5: exactly 10.0, the floor
    floor = float(thr[0])
    # the inputs, on the fake scan alone: enough entries, a site and a storm with none, a value exactly at the floor
    m = plane(slon, slat)
    with np.errstate(invalid='ignore'):
        kept = m >= floor
    assert kept.sum() >= 200 and (~kept).all(axis=1).any() and (~kept).all(axis=0).any() and m[40, 5] == floor and kept[40, 5]
    assert (~np.isnan(m) & ~kept).sum() >= 10                         # and values below it that are not NaN
    blocked = events.site_event_table(scan, slon, slat, floor, max_bytes=1)
    assert [c[0].size for c in calls] == [64, 64, 2]                   # 130 sites: the last block is ragged
    order = spatial_order(slon, slat, np)
    assert np.array_equal(np.concatenate([c[0] for c in calls]), slon[order])          # the sites went in spatial order, once
    assert np.array_equal(np.concatenate([c[1] for c in calls]), slat[order])
    del calls[:]
    one = events.site_event_table(scan, slon, slat, floor, n_trk=37)
    assert [c[0].size for c in calls] == [130]
    del calls[:]
    probe = events.site_event_table(scan, slon, slat, floor, max_bytes=8 * 37 * 100)       # n_trk unknown: 64 sites, then 64 more
    assert [c[0].size for c in calls] == [64, 64, 2]
    # the expected table, in the caller's order, without the driver
    want = EN.row_pack(m, floor)
    direct = scan(slon, slat)
    for res in (blocked, one, probe):
        assert _same_csr((res['site_ptr'], res['storm'], res['value']), want)
        assert res['n_trk'] == 37 and res['min_value'] == floor and res['key'] == 'site_max'
        assert res['counts'].dtype == np.int32 and np.array_equal(res['counts'], direct['counts']) and np.array_equal(res['thresholds'], thr)
        assert _same_table(res, blocked)
        assert same_bits(events.dense(res), np.where(kept, m, np.nan)) and same_bits(events.dense(res), EN.dense(res))
        got = events.counts_from_table(res, groups, 4, thr)
        assert got.dtype == np.int32 and np.array_equal(got, direct['counts']) and np.array_equal(got, EN.counts_from_table(res, groups, 4, thr))
        ev, ev_want = events.by_storm(res), EN.by_storm(res)
        assert ev['storm_ptr'].dtype == np.int64 and ev['site'].dtype == np.int32 and ev['storm_ptr'].shape == (38,)
        assert np.array_equal(ev['storm_ptr'], ev_want['storm_ptr']) and np.array_equal(ev['site'], ev_want['site'])
        assert same_bits(ev['value'], ev_want['value'])
    assert blocked['site_ptr'][18] == blocked['site_ptr'][17]          # the unreachable site has no entry
    ev = events.by_storm(blocked)
    assert ev['storm_ptr'][8] == ev['storm_ptr'][7]                    # and storm 7 has none


def test_counts_from_table_refuses_a_threshold_below_the_floor():
    from tropical_cyclone_risk_amd import events
    table = dict(site_ptr=np.array([0, 2, 2, 5]), storm=np.array([1, 3, 0, 1, 2], np.int32), value=np.array([20.0, 30.0, 12.0, 40.0, 10.0]),
                 n_trk=4, min_value=10.0)
    groups = np.array([0, 1, 1, 0])
    assert events.counts_from_table(table, groups, 2, [10.0, 25.0]).tolist() == [[[1, 1], [1, 0]], [[0, 0], [0, 0]], [[1, 0], [2, 1]]]
    for bad in ([9.999, 25.0], [-np.inf], [np.nan], []):
        with pytest.raises(ValueError):
            events.counts_from_table(table, groups, 2, bad)
    with pytest.raises(ValueError):
        events.counts_from_table(table, groups[:3], 2, [10.0])
    with pytest.raises(ValueError):
        events.dense(dict(table, site_ptr=np.zeros(2 ** 14 + 2, np.int64), storm=table['storm'][:0], value=table['value'][:0], n_trk=2 ** 14))


def test_save_and_load_round_trip(tmp_path):
    from tropical_cyclone_risk_amd import events
    table = dict(site_ptr=np.array([0, 2, 2, 5]), storm=np.array([1, 3, 0, 1, 2], np.int32), value=np.array([20.0, -0.0, 12.0, np.inf, 10.0]),
                 n_trk=4, min_value=-0.0, key='site_total', counts=np.zeros((3, 1, 1), np.int32), thresholds=np.array([0.0]))
    lon, lat = np.array([280.0, 281.0, 282.5]), np.array([20.0, 21.0, 22.0])
    fn = str(tmp_path / 'ev.npz')
    events.save_events(fn, table, lon, lat, unit='mm', storm_year=np.array([2001, 2001, 2003, 2003]), storm_file=np.zeros(4, np.int64))
    z = events.load_events(fn)
    assert set(z) == {'site_ptr', 'storm', 'value', 'site_lon', 'site_lat', 'n_trk', 'min_value', 'key', 'unit', 'storm_year', 'storm_file'}
    assert _same_csr((z['site_ptr'], z['storm'], z['value']), (table['site_ptr'], table['storm'], table['value']))
    assert z['n_trk'] == 4 and isinstance(z['n_trk'], int) and z['min_value'] == 0.0 and np.signbit(z['min_value'])
    assert z['key'] == 'site_total' and z['unit'] == 'mm' and z['storm_year'].tolist() == [2001, 2001, 2003, 2003]
    assert np.array_equal(z['site_lon'], lon) and np.array_equal(z['site_lat'], lat)
    assert same_bits(events.dense(z), EN.dense(table))                 # what was loaded is a table the views take
    import zipfile
    with zipfile.ZipFile(fn) as f:
        assert all(i.compress_type == zipfile.ZIP_STORED for i in f.infolist())        # uncompressed
    with pytest.raises(ValueError):
        events.save_events(fn, table, lon[:2], lat[:2])
    with pytest.raises(ValueError):
        events.save_events(fn, table, lon, lat, value=np.zeros(5))


def test_cli_options_are_off_by_default():
    from tropical_cyclone_risk_amd import hazard, rainfall, windfield
    for mod in (hazard, windfield, rainfall):
        a = mod.parse_args(['x.nc', '--site', '1,2'])
        assert a.events_out is None and a.events_min is None
        a = mod.parse_args(['x.nc', '--site', '1,2', '--events-out', 'e.npz', '--events-min', '17.5'])
        assert a.events_out == 'e.npz' and a.events_min == 17.5
        assert mod.parse_args(['x.nc', '--site', '1,2', '--events-out', 'e.npz', '--events-min=-inf']).events_min == -np.inf
        for bad in (['--events-out', 'e.npz'], ['--events-min', '5'], ['--events-out', 'e.npz', '--events-min', 'nan'],
                    ['--events-out', 'e.npz', '--events-min', 'x'], ['--events-out', 'e.npz', '--events-min', '']):
            with pytest.raises(SystemExit):
                mod.parse_args(['x.nc', '--site', '1,2'] + bad)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _both_entry_points(buf, n_col, floor):
    """row_pack on the [n_row][n_col] view of buf [n_row][row_stride] through tcr_rowpack_host (NumPy) and the two _dev calls
    (torch); the view is read where it lies: the columns past n_col never appear."""
    import torch
    from tropical_cyclone_risk_amd import events
    view = buf[:, :n_col]
    want = EN.row_pack(view, floor)
    assert not view.flags['C_CONTIGUOUS'] or buf.shape[1] == n_col or buf.shape[0] <= 1
    assert _same_csr(events.row_pack(view, floor), want), 'tcr_rowpack_host'
    t = torch.as_tensor(buf, device=torch.device('cuda', 0))[:, :n_col]
    assert t.stride() == (buf.shape[1], 1)
    got = events.row_pack(t, floor)
    assert all(a.device == t.device for a in got) and got[0].dtype == torch.int64 and got[1].dtype == torch.int32
    assert _same_csr(tuple(a.cpu().numpy() for a in got), want), 'tcr_rowpack_dev'
    return want


def _density_rows(rng, n_col, floor, turn):
    """Six rows: nothing kept, everything kept, lanes 0 and 63 of every wave only, the last turn of the workgroup only, about 1 %
    and about 50 % at random.  What is not kept is NaN or a value below the floor; some kept values are the floor itself."""
    c = np.arange(n_col)
    last = (n_col - 1) // turn * turn
    keep = np.stack([np.zeros(n_col, bool), np.ones(n_col, bool), (c % 64 == 0) | (c % 64 == 63), (c >= last) if last else (c == n_col - 1),
                     rng.random(n_col) < 0.01, rng.random(n_col) < 0.5])
    high = floor + np.where(rng.random(keep.shape) < 0.2, 0.0, np.abs(rng.normal(0.0, 15.0, keep.shape)))
    low = np.where(rng.random(keep.shape) < 0.5, np.nan, floor - np.abs(rng.normal(0.0, 15.0, keep.shape)) - 1e-9)
    return np.where(keep, high, low), keep


def _shape_cases():
    from tropical_cyclone_risk_amd import _lib
    turn = 256 * _lib.ROWPACK_UNROLL
    return [1, 63, 64, 65, 255, 256, 257, turn - 1, turn, turn + 1, 5000]


@pytest.mark.gpu
@pytest.mark.parametrize('n_col', _shape_cases())
def test_gpu_shapes_and_densities_with_a_row_stride(built_lib, n_col):
    from tropical_cyclone_risk_amd import _lib
    rng = np.random.default_rng(200 + n_col)
    floor = 17.5
    rows, keep = _density_rows(rng, n_col, floor, 256 * _lib.ROWPACK_UNROLL)
    rows[1, 0] = floor                                                     # a value exactly at the floor, whatever the draw
    buf = np.empty((6, n_col + 3))
    buf[:, :n_col] = rows
    buf[:, n_col:] = 1e9 + rng.random((6, 3))                              # finite decoys in the gap, above the floor
    ptr, col, val = _both_entry_points(buf, n_col, floor)
    assert np.array_equal(np.diff(ptr), keep.sum(axis=1)) and ptr[1] == 0 and ptr[2] == n_col
    assert (val < 1e8).all() and (col < n_col).all() and (val == floor).any()


@pytest.mark.gpu
def test_gpu_special_values_at_every_floor(built_lib):
    rng = np.random.default_rng(7)
    n_col = 300
    rows = np.stack([SPECIAL[rng.permutation(np.resize(np.arange(SPECIAL.size), n_col))] for _ in range(3)] + [np.resize(SPECIAL, n_col)])
    for floor, cols in SPECIAL_KEPT:
        ptr, col, val = _both_entry_points(np.ascontiguousarray(rows), n_col, floor)
        assert ptr[4] - ptr[3] == len(cols) * (n_col // SPECIAL.size), floor
        assert col[ptr[3]:ptr[3] + len(cols)].tolist() == cols and same_bits(val[ptr[3]:ptr[3] + len(cols)], SPECIAL[cols])
        assert not np.isnan(val).any()
    ptr, col, val = _both_entry_points(np.ascontiguousarray(rows), n_col, 0.0)
    assert np.signbit(val[val == 0.0]).any() and not np.signbit(val[val == 0.0]).all()           # both zeros kept, each as it was
    one = np.full((1, 100), np.nan)                                        # one row: the stride does not matter
    one[0, 99] = -7.25
    assert _both_entry_points(one, 100, -np.inf)[1].tolist() == [99]


@pytest.mark.gpu
def test_gpu_many_short_rows(built_lib):
    rng = np.random.default_rng(23)
    plane = np.round(rng.normal(0.0, 3.0, (70000, 8)), 1)                   # more rows than the grid cap; ties, and both zeros
    plane[rng.random(plane.shape) < 0.3] = np.nan
    plane[plane == 0.0] *= rng.choice([1.0, -1.0], (plane == 0.0).sum())
    ptr, col, val = _both_entry_points(plane, 8, 0.0)
    assert set(np.unique(np.diff(ptr))) == set(range(9)) and ptr[-1] == col.size > 100000


def _ctx():
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    return L, h


@pytest.mark.gpu
def test_gpu_no_rows(built_lib):
    import torch
    L, h = _ctx()
    try:
        ptr = np.full(3, -1, np.int64)
        assert L.tcr_rowpack_host(h, None, 0, 4, 4, 1.0, ptr.ctypes.data, 0, None, None) == 0 and ptr.tolist() == [0, -1, -1]
        dev = torch.device('cuda', 0)
        tp = torch.full((3,), -1, dtype=torch.int64, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        assert L.tcr_rowpack_count_dev(h, None, 0, 4, 4, 1.0, tp.data_ptr(), st) == 0
        assert L.tcr_rowpack_fill_dev(h, None, 0, 4, 4, 1.0, tp.data_ptr(), 0, None, None, st) == 0
        assert tp.cpu().tolist() == [0, -1, -1]
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_fill_never_writes_at_or_past_capacity(built_lib):
    """No fault is sought: the buffers are valid and longer than the capacity."""
    import torch
    L, h = _ctx()
    try:
        rng = np.random.default_rng(41)
        n_row, n_col, floor = 6, 5000, 17.5
        plane = np.where(rng.random((n_row, n_col)) < 0.5, rng.normal(40.0, 10.0, (n_row, n_col)), np.nan)
        want = EN.row_pack(plane, floor)
        nnz = int(want[0][-1])
        assert nnz > 1000
        dev = torch.device('cuda', 0)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        tp, tr = torch.as_tensor(plane, device=dev), torch.empty(n_row + 1, dtype=torch.int64, device=dev)
        tc, tv = torch.full((nnz,), -7, dtype=torch.int32, device=dev), torch.full((nnz,), -7.0, dtype=torch.float64, device=dev)
        assert L.tcr_rowpack_count_dev(h, tp.data_ptr(), n_row, n_col, n_col, floor, tr.data_ptr(), st) == 0
        assert np.array_equal(tr.cpu().numpy(), want[0])
        assert L.tcr_rowpack_fill_dev(h, tp.data_ptr(), n_row, n_col, n_col, floor, tr.data_ptr(), nnz - 5, tc.data_ptr(), tv.data_ptr(), st) == 0
        col, val = tc.cpu().numpy(), tv.cpu().numpy()
        assert np.array_equal(col[:-5], want[1][:-5]) and same_bits(val[:-5], want[2][:-5])
        assert (col[-5:] == -7).all() and (val[-5:] == -7.0).all()
        # the host entry point reports it, with the right row_ptr and the buffers untouched
        ptr, hc, hv = np.full(n_row + 1, -1, np.int64), np.full(nnz, -7, np.int32), np.full(nnz, -7.0)
        assert L.tcr_rowpack_host(h, plane.ctypes.data, n_row, n_col, n_col, floor, ptr.ctypes.data, nnz - 5, hc.ctypes.data, hv.ctypes.data) == -1
        msg = L.tcr_last_error(h).decode()
        assert msg.startswith('tcr_rowpack:') and 'capacity' in msg, msg
        assert np.array_equal(ptr, want[0]) and (hc == -7).all() and (hv == -7.0).all()
        assert L.tcr_rowpack_host(h, plane.ctypes.data, n_row, n_col, n_col, floor, ptr.ctypes.data, nnz, hc.ctypes.data, hv.ctypes.data) == 0
        assert _same_csr((ptr, hc, hv), want)
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_abi_rejects_bad_arguments(built_lib):
    import torch
    L, h = _ctx()
    try:
        plane = np.arange(12.0).reshape(3, 4)
        ptr, col, val = np.full(4, -1, np.int64), np.full(12, -1, np.int32), np.full(12, -1.0)

        def call(n_row=3, n_col=4, stride=4, floor=5.0, cap=12, plane_=plane, ptr_=ptr, col_=col, val_=val):
            p = lambda a: None if a is None else a.ctypes.data              # noqa: E731
            return L.tcr_rowpack_host(h, p(plane_), n_row, n_col, stride, floor, p(ptr_), cap, p(col_), p(val_))
        for bad in (dict(floor=np.nan), dict(floor=float(NEG_NAN)), dict(stride=3), dict(n_col=0), dict(n_col=2 ** 31), dict(cap=-1),
                    dict(n_row=-1), dict(plane_=None), dict(ptr_=None), dict(col_=None), dict(val_=None, cap=0)):
            assert call(**bad) == -1, bad
            assert L.tcr_last_error(h).decode().startswith('tcr_rowpack:'), (bad, L.tcr_last_error(h))
        assert (ptr == -1).all() and (col == -1).all() and (val == -1.0).all()         # none of them wrote anything
        dev = torch.device('cuda', 0)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        tp, tr = torch.as_tensor(plane, device=dev), torch.full((4,), -1, dtype=torch.int64, device=dev)
        tc, tv = torch.full((12,), -1, dtype=torch.int32, device=dev), torch.full((12,), -1.0, dtype=torch.float64, device=dev)
        for floor, n_col, stride in ((np.nan, 4, 4), (5.0, 0, 4), (5.0, 4, 3)):
            assert L.tcr_rowpack_count_dev(h, tp.data_ptr(), 3, n_col, stride, floor, tr.data_ptr(), st) == -1
            assert L.tcr_last_error(h).decode().startswith('tcr_rowpack:')
            assert L.tcr_rowpack_fill_dev(h, tp.data_ptr(), 3, n_col, stride, floor, tr.data_ptr(), 12, tc.data_ptr(), tv.data_ptr(), st) == -1
            assert L.tcr_last_error(h).decode().startswith('tcr_rowpack:')
        assert L.tcr_rowpack_fill_dev(h, tp.data_ptr(), 3, 4, 4, 5.0, tr.data_ptr(), -1, tc.data_ptr(), tv.data_ptr(), st) == -1
        assert L.tcr_last_error(h).decode().startswith('tcr_rowpack:')
        assert (tr.cpu() == -1).all() and (tc.cpu() == -1).all() and (tv.cpu() == -1.0).all()
        assert call() == 0 and ptr.tolist() == [0, 0, 3, 7] and col[:7].tolist() == [1, 2, 3, 0, 1, 2, 3] and val[:7].tolist() == [5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]
        assert call(cap=0, col_=None, val_=None, floor=-np.inf) == 0 and ptr.tolist() == [0, 4, 8, 12]          # counting only
    finally:
        L.tcr_ctx_destroy(h)


def _small_ensemble(rng, n_trk=40, n_t=30):
    """The ensemble shape of test_levels._small_ensemble: random walks in one box, hourly, some with NaN tails; 130 sites in and
    around the box, three far away; 10 groups (years)."""
    lon = rng.uniform(280, 300, (n_trk, 1)) + np.cumsum(rng.normal(-0.1, 0.15, (n_trk, n_t)), axis=1)
    lat = rng.uniform(15, 35, (n_trk, 1)) + np.cumsum(rng.normal(0.08, 0.1, (n_trk, n_t)), axis=1)
    v = np.clip(30 + np.cumsum(rng.normal(0.2, 1.5, (n_trk, n_t)), axis=1), 12, 80)
    env = [rng.normal(0, 6, (n_trk, n_t)) for _ in range(4)]
    end = rng.integers(4, n_t + 1, n_trk)
    for p in [lon, lat, v] + env:
        p[np.arange(n_t)[None, :] >= end[:, None]] = np.nan
    slon, slat = rng.uniform(276, 302, 130), rng.uniform(12, 40, 130)
    slon[[3, 77, 129]], slat[[3, 77, 129]] = [100.0, 20.0, -170.0], [-30.0, 60.0, 5.0]          # no storm reaches these
    return lon, lat, v, env, rng.integers(0, 10, n_trk), slon, slat


def _check_events_of_a_scan(scan, plane_key, slon, slat, n_trk, thr, groups):
    """site_event_table at the floor thresholds[0] in 64-site blocks (twice) and in one block: identical, the scan's own unblocked
    plane masked at the floor, and the scan's own counts, without a tolerance."""
    from tropical_cyclone_risk_amd import events
    from tropical_cyclone_risk_amd.analysis import to_numpy
    floor = float(thr[0])
    sizes = []

    def counted(x, y):
        sizes.append(int(x.shape[0]))
        return scan(x, y)

    def table(**kw):
        res = events.site_event_table(counted, slon, slat, floor, key=plane_key, **kw)
        dense, counts, ev = events.dense(res), events.counts_from_table(res, groups, 10, thr), events.by_storm(res)
        out = {n: to_numpy(a) if hasattr(a, 'shape') else a for n, a in res.items()}
        return out, to_numpy(dense), to_numpy(counts), {n: to_numpy(a) for n, a in ev.items()}
    blocked, again, one = table(max_bytes=1), table(max_bytes=1), table(n_trk=n_trk)
    assert sizes == [64, 64, 2, 64, 64, 2, 130]
    direct = scan(slon, slat)
    m, counts = to_numpy(direct[plane_key]), to_numpy(direct['counts'])
    with np.errstate(invalid='ignore'):
        kept = m >= floor
    assert kept.sum() >= 50 and (~kept).all(axis=1).sum() >= 3 and (~np.isnan(m) & ~kept).any(), kept.sum()
    want = EN.row_pack(m, floor)
    for res, dense, got_counts, ev in (blocked, again, one):
        assert _same_table(res, blocked[0]) and res['n_trk'] == n_trk and res['key'] == plane_key
        assert _same_csr((res['site_ptr'], res['storm'], res['value']), want)
        assert same_bits(dense, np.where(kept, m, np.nan))
        assert got_counts.dtype == np.int32 and np.array_equal(got_counts, counts) and np.array_equal(res['counts'], counts)
        ev_want = EN.by_storm(res)
        assert np.array_equal(ev['storm_ptr'], ev_want['storm_ptr']) and np.array_equal(ev['site'], ev_want['site'])
        assert ev['site'].dtype == np.int32 and same_bits(ev['value'], ev_want['value'])


@pytest.mark.gpu
def test_gpu_events_of_the_wind_footprint_against_its_own_plane_and_counts(built_lib):
    import torch
    from tropical_cyclone_risk_amd import windfield
    lon, lat, v, env, groups, slon, slat = _small_ensemble(np.random.default_rng(31))
    dev = torch.device('cuda', 0)
    tl, ta, tv, sl, sa = (torch.as_tensor(x, device=dev) for x in (lon, lat, v, slon, slat))
    tenv = [torch.as_tensor(x, device=dev) for x in env]
    thr = np.arange(10.0, 71.0, 5.0)

    def scan(x, y):
        return windfield.site_wind(tl, ta, tv, tenv, groups, x, y, 3600.0, thresholds=thr, return_max=True, n_groups=10)
    _check_events_of_a_scan(scan, 'site_max', sl, sa, lon.shape[0], thr, groups)


@pytest.mark.gpu
@pytest.mark.parametrize('stat', ['total', 'peak-rate'])
def test_gpu_events_of_the_rainfall_against_its_own_plane_and_counts(built_lib, stat):
    """The NumPy flavour: every block crosses to the device and back through tcr_rowpack_host."""
    from tropical_cyclone_risk_amd import rainfall
    lon, lat, v, env, groups, slon, slat = _small_ensemble(np.random.default_rng(37))
    thr = np.array([1.0, 5.0, 10.0, 25.0, 50.0, 100.0, 200.0]) if stat == 'total' else np.array([0.5, 1.0, 2.0, 4.0, 8.0, 12.0])

    def scan(x, y):
        return rainfall.site_rain(lon, lat, v, groups, x, y, 3600.0, stat=stat, thresholds=thr, return_values=True, n_groups=10)
    _check_events_of_a_scan(scan, rainfall.STATS[stat][1], slon, slat, lon.shape[0], thr, groups)


def _nl(**over):
    from tropical_cyclone_risk_amd import namelist
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    for k, val in over.items():
        setattr(nl, k, val)
    return nl


def _write_track_file(tmp_path, rng):
    """Three years with 6, 0 and 7 storms in one file written by io.write_tracks, on the namelist's time axis (as
    test_levels._write_track_file)."""
    from tropical_cyclone_risk_amd import io as tio
    from tropical_cyclone_risk_amd.basins import TC_Basin
    nl = _nl(output_directory=str(tmp_path), exp_name='ev', start_year=2001, end_year=2003)
    ns = int(nl.total_track_time_days * 24 * 60 * 60 / nl.output_interval_s) + 1

    def year(n):
        lon = rng.uniform(282, 290, (n, 1)) + np.cumsum(rng.normal(-0.02, 0.03, (n, ns)), axis=1)
        lat = rng.uniform(20, 28, (n, 1)) + np.cumsum(rng.normal(0.02, 0.02, (n, ns)), axis=1)
        v = np.clip(25 + np.cumsum(rng.normal(0.05, 0.6, (n, ns)), axis=1), 10, 75)
        env = rng.normal(0, 5, (n, ns, 4))
        end = rng.integers(ns // 3, ns + 1, n)
        tail = np.arange(ns)[None, :] >= end[:, None]
        for p in (lon, lat, v):
            p[tail] = np.nan
        env[tail] = np.nan
        return (lon, lat, v, v, v + 3.0, env, rng.integers(1, 13, n).astype(float), np.array(['NA'] * n, dtype='U2'),
                rng.integers(0, 9, (7, 12)).astype(float))
    return tio.write_tracks([year(6), year(0), year(7)], [2001, 2002, 2003], TC_Basin('NA'), nl)


@pytest.mark.gpu
def test_gpu_cli_round_trip(built_lib, tmp_path, capsys):
    """--events-out FILE --events-min V writes the table of hazard, windfield and rainfall beside the .npz, which keeps its keys; the
    file loads, and its table is the library call's."""
    from tropical_cyclone_risk_amd import analysis, events, hazard, rainfall, windfield
    fn = _write_track_file(tmp_path, np.random.default_rng(5))
    sites0 = ['--site=-75.0,24.0', '--site', '286.5,25.5', '--site=-72.25,27.0', '--site', '10.0,50.0']
    lon, lat, vmax, v, env, groups, gfile, gyear, dt = analysis.load_wind_planes([fn])
    assert lon.shape[0] == 13
    for mod, key, unit, floor, more, call in (
            (hazard, 'site_max', 'm/s', '15', ['--radius-km', '400'],
             lambda x, y: hazard.site_hazard(lon, lat, vmax, groups, x, y, radius_km=400.0, return_max=True, n_groups=3)),
            (windfield, 'site_max', 'm/s', '12.5', [],
             lambda x, y: windfield.site_wind(lon, lat, v, env, groups, x, y, dt, return_max=True, n_groups=3)),
            (rainfall, 'site_total', 'mm', '1', [],
             lambda x, y: rainfall.site_rain(lon, lat, vmax, groups, x, y, dt, return_values=True, n_groups=3))):
        name = mod.__name__.split('.')[-1]
        out, ev = str(tmp_path / (name + '.npz')), str(tmp_path / (name + '_events.npz'))
        sites = sites0 + more
        assert mod.main([fn, '--out', out] + sites) == 0
        plain = set(np.load(out).files)
        assert not os.path.exists(ev) and 'largest events' not in capsys.readouterr().out
        assert mod.main([fn, '--out', out, '--events-out', ev, '--events-min', floor] + sites) == 0
        assert set(np.load(out).files) == plain, name
        assert 'largest events' in capsys.readouterr().out
        z = events.load_events(ev)
        assert set(z) == {'site_ptr', 'storm', 'value', 'site_lon', 'site_lat', 'n_trk', 'min_value', 'key', 'unit', 'storm_year',
                          'storm_file', 'files'}, name
        want = events.site_event_table(call, z['site_lon'], z['site_lat'], float(floor), key=key)
        assert _same_csr((z['site_ptr'], z['storm'], z['value']), (want['site_ptr'], want['storm'], want['value'])), name
        assert z['n_trk'] == 13 and z['min_value'] == float(floor) and z['key'] == key and z['unit'] == unit
        assert z['storm_year'].tolist() == [2001] * 6 + [2003] * 7 and (z['storm_file'] == 0).all() and z['site_ptr'].shape == (5,)
        n = np.diff(z['site_ptr'])
        assert n[3] == 0 and n.sum() >= 3, (name, n)
