"""Joint site hazard (tropical_cyclone_risk_amd/joint.py, csrc/tcr_joint.hip): one bit per (site, level, unit) of a per-storm plane,
and the co-exceedance counts between sites as popcounts of ANDed bit rows.  CPU tests pin the restatement (tests/joint_numpy.py) to
hand values and check the argument handling, the blocked driver on a scan made of NumPy, the pure functions and the command line's
parser; GPU tests (`-m gpu`) check the kernels against the restatement through both entry points, and joint_hazard against the
plane and the counts of the scan it comes from.  Every result is an integer: nothing here has a tolerance."""
import ctypes
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import joint_numpy as JN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_NAN = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]        # a NaN with the sign bit set (and a payload)
#                       0    1     2       3       4        5    6     7        8       9        10    11
SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3.5, -3.5, NEG_NAN, 1e-310, -1e-310, 17.5, 17.5])
SPECIAL_REACH = ((0.0, [0, 1, 3, 5, 8, 10, 11]), (-0.0, [0, 1, 3, 5, 8, 10, 11]), (-np.inf, [0, 1, 3, 4, 5, 6, 8, 9, 10, 11]),
                 (np.inf, [3]), (17.5, [3, 10, 11]), (3.5, [3, 5, 10, 11]))


def _word(cols):
    return sum(1 << c for c in cols)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_by_hand():
    assert np.isnan(NEG_NAN) and np.signbit(NEG_NAN)
    levels = [lev for lev, _ in SPECIAL_REACH]
    bits, n_set = JN.pack_bits(SPECIAL[None, :], levels)
    assert bits.shape == (6, 1, 1) and bits.dtype == np.uint64 and n_set.dtype == np.int32
    for l, (lev, cols) in enumerate(SPECIAL_REACH):
        assert int(bits[l, 0, 0]) == _word(cols) and n_set[l, 0] == len(cols), lev
    # a 3 x 4 plane, one level per row and one for all: the words and the counts written by hand
    plane = np.array([[1.0, 5.0, np.nan, 7.0], [6.0, 5.0, 4.0, np.nan], [np.nan, 9.0, 9.0, 9.0]])
    bits, n_set = JN.pack_bits(plane, [5.0])
    assert bits[0, :, 0].tolist() == [0b1010, 0b0011, 0b1110] and n_set.tolist() == [[2, 2, 3]]
    assert JN.cross_counts(bits).tolist() == [[[2, 1, 2], [1, 2, 1], [2, 1, 3]]]
    assert JN.cross_counts(bits[:, [2]], bits).tolist() == [[[2, 1, 3]]]
    bits, n_set = JN.pack_bits(plane, [[7.0, 1.0], [4.0, 6.0], [-np.inf, 10.0]])
    assert bits[:, :, 0].tolist() == [[0b1000, 0b0111, 0b1110], [0b1011, 0b0001, 0]] and n_set.tolist() == [[1, 3, 3], [3, 1, 0]]
    j, n = JN.joint(plane, [[7.0, 1.0], [4.0, 6.0], [-np.inf, 10.0]])
    assert j.tolist() == [[[1, 0, 1], [0, 3, 2], [1, 2, 3]], [[3, 1, 0], [1, 1, 0], [0, 0, 0]]] and np.array_equal(n, n_set)
    # the mapped mode: unit 1 is empty, unit 2 holds three storms, the order is arbitrary
    unit_of = np.array([2, 0, 2, 2])
    bits, n_set = JN.pack_bits(plane, [5.0], unit_of, 4)
    assert bits[0, :, 0].tolist() == [0b0101, 0b0101, 0b0101] and n_set.tolist() == [[2, 2, 2]]
    bits, n_set = JN.pack_bits(plane, [8.0], unit_of, 4)
    assert bits[0, :, 0].tolist() == [0, 0, 0b0101] and n_set.tolist() == [[0, 0, 2]]
    # more than one word: unit 64 is bit 0 of word 1, and the bits past n_unit stay zero
    row = np.full((1, 70), np.nan)
    row[0, [0, 63, 64, 69]] = 1.0
    bits, n_set = JN.pack_bits(row, [1.0])
    assert bits[0, 0].tolist() == [1 | 1 << 63, 1 | 1 << 5] and n_set.tolist() == [[4]]
    assert np.array_equal(JN.unpack(bits, 70), JN.exceed(row, [1.0]))


def test_joint_symbols_exported_constants_and_abi_version_unchanged(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_joint_pack_dev', 'tcr_joint_cross_dev', 'tcr_joint_host'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    L.tcr_abi_version.restype = ctypes.c_int
    assert L.tcr_abi_version() == 7 and _lib.TCR_ABI_VERSION == 7
    src = ('#include <stdio.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%d %d %d\\n",TCR_JOINT_MAX_LEVELS,'
           'TCR_JOINT_MAX_MAPPED_UNITS,TCR_JOINT_KW);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'k.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'k')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [_lib.JOINT_MAX_LEVELS, _lib.JOINT_MAX_MAPPED_UNITS, _lib.JOINT_KW] == [16, 2 ** 18, got[2]] and got[2] >= 2


def test_argument_errors_before_any_device_work(monkeypatch):
    from tropical_cyclone_risk_amd import _lib, joint

    def no_library():
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', no_library)
    plane = np.arange(12.0).reshape(3, 4)
    for lev in ([np.nan], [1.0, NEG_NAN], 5.0, np.zeros((1, 3, 1)), np.zeros((4, 2)), np.zeros((2, 2)), [], np.zeros((3, 0)),
                np.arange(17.0), np.zeros((3, 17)), 'x'):
        with pytest.raises(ValueError):
            joint.pack_bits(plane, lev)
    for kw in (dict(unit_of=[0, 1, 2, 4], n_unit=4), dict(unit_of=[0, 1, -1, 2], n_unit=4), dict(unit_of=[0, 1, 2]), dict(unit_of=[0, 1, 2, 3, 0]),
               dict(unit_of=[0.0, 1.0, 2.0, 3.0]), dict(unit_of=[0, 1, 2, 3], n_unit=0), dict(unit_of=[0, 1, 2, 3], n_unit=2 ** 18 + 1),
               dict(n_unit=5)):
        with pytest.raises(ValueError):
            joint.pack_bits(plane, [1.0], **kw)
    for bad in (np.arange(4.0), np.zeros((3, 0)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            joint.pack_bits(bad, [1.0])
    for a, b in ((np.zeros((2, 3), np.uint64), None), (np.zeros((1, 2, 3)), None), (np.zeros((17, 2, 3), np.uint64), None),
                 (np.zeros((1, 2, 3), np.uint64), np.zeros((1, 2, 4), np.uint64)), (np.zeros((1, 2, 3), np.uint64), np.zeros((2, 2, 3), np.uint64))):
        with pytest.raises(ValueError):
            joint.cross_counts(a, b)
    bits, n_set = joint.pack_bits(np.zeros((0, 70)), [1.0, 2.0])            # no rows: nothing to ask the library
    assert bits.shape == (2, 0, 2) and bits.dtype == np.uint64 and n_set.shape == (2, 0) and n_set.dtype == np.int32
    assert joint.cross_counts(bits, np.zeros((2, 3, 2), np.uint64)).shape == (2, 0, 3)
    with pytest.raises(AssertionError, match='the library was touched'):
        joint.pack_bits(plane, [1.0])
    with pytest.raises(AssertionError, match='the library was touched'):
        joint.cross_counts(np.zeros((1, 2, 3), np.uint64))

    def scan(x, y):
        raise AssertionError('the scan was called before the arguments were checked')
    lon, lat = np.array([280.0, 281.0, 282.0]), np.array([20.0, 21.0, 22.0])
    ok = dict(scan=scan, site_lon=lon, site_lat=lat, levels=[30.0, 50.0])
    for kw in (dict(levels=[np.nan]), dict(levels=np.zeros((2, 2))), dict(levels=[]), dict(levels=np.arange(17.0)), dict(levels=np.zeros((3, 17))),
               dict(unit='group'), dict(unit='year'), dict(unit='group', groups=[0, -1]), dict(unit='group', groups=[0, 3], n_groups=3),
               dict(unit='group', groups=[0, 1], n_trk=3), dict(unit='group', groups=[0, 1], n_groups=2 ** 18 + 1),
               dict(anchors=[3]), dict(anchors=[-1]), dict(anchors=[]), dict(anchors=[0.0]), dict(anchors=[[0]]),
               dict(max_out_bytes=2 * 3 * 3 * 4 - 1), dict(anchors=[1], max_out_bytes=2 * 3 * 4 - 1), dict(max_bytes=0), dict(site_lat=lat[:1]),
               dict(site_lon=np.array([np.inf, 1.0, 2.0]))):
        with pytest.raises(ValueError):
            joint.joint_hazard(**dict(ok, **kw))
    with pytest.raises(ValueError, match='choose anchors'):
        joint.joint_hazard(**dict(ok, max_out_bytes=10))
    for kw in ({}, dict(anchors=[1], max_out_bytes=2 * 3 * 4), dict(unit='group', groups=[0, 1, 1, 0])):
        with pytest.raises(AssertionError, match='the scan was called'):
            joint.joint_hazard(**dict(ok, **kw))


def _fake_scan(rng, n_trk=37, n_groups=4):
    """A site analysis made of NumPy (the idea of test_events._fake_scan): storm s is a disc of radius r_s degrees around (cx_s,
    cy_s) with peak p_s, and a site's value of it falls off with the distance (NaN outside).  A site's row depends on that site
    alone, as in the real scans."""
    cx, cy, rad, peak = rng.uniform(270, 300, n_trk), rng.uniform(10, 40, n_trk), rng.uniform(4, 14, n_trk), rng.uniform(15, 80, n_trk)
    groups = rng.integers(0, n_groups, n_trk)
    thr = np.array([10.0, 20.0, 30.0, 50.0])
    calls = []

    def plane(x, y):
        d = np.hypot(x[:, None] - cx[None, :], y[:, None] - cy[None, :])
        return np.where(d <= rad[None, :], peak[None, :] * (1.0 - 0.06 * d), np.nan)

    def scan(x, y):
        calls.append((np.array(x), np.array(y)))
        m = plane(np.asarray(x), np.asarray(y))
        counts = np.zeros((m.shape[0], n_groups, thr.size), np.int32)
        for g in range(n_groups):
            counts[:, g] = (m[:, groups == g, None] >= thr[None, None, :]).sum(axis=1)
        return dict(counts=counts, thresholds=thr, site_max=m)
    return scan, plane, calls, thr, groups


def test_blocked_driver_equals_the_unblocked_result_in_the_callers_site_order(monkeypatch):
    from tropical_cyclone_risk_amd import joint
    from tropical_cyclone_risk_amd.sitescan import spatial_order
    monkeypatch.setattr(joint, 'pack_bits', JN.pack_bits)
    monkeypatch.setattr(joint, 'cross_counts', JN.cross_counts)
    rng = np.random.default_rng(19)
    scan, plane, calls, thr, groups = _fake_scan(rng)
    slon, slat = rng.uniform(268, 302, 130), rng.uniform(8, 42, 130)        # (drawn at random: the caller's order is shuffled in space)
    slon[17], slat[17] = 100.0, -30.0                                      # no storm reaches this one
    order = spatial_order(slon, slat, np)
    assert not np.array_equal(order, np.arange(130))
    m = plane(slon, slat)
    direct = scan(slon, slat)
    del calls[:]
    per_site = np.stack([rng.uniform(15, 35, 130), rng.uniform(30, 60, 130)], axis=1)
    anchors = np.array([40, 17, 3, 129, 40])                               # any order, a repeat, the unreachable site
    for levels in ([20.0, 30.0, 50.0], per_site):
        for unit, kw, map_ in (('storm', {}, {}), ('group', dict(groups=groups, n_groups=5), dict(unit_of=groups, n_unit=5))):
            want, want_set = JN.joint(m, levels, anchors, **map_)
            assert want.sum() > 100 and (want_set[:, 17] == 0).all() and (want[:, 1] == 0).all()
            results = []
            for blocks, size in (([64, 64, 2], dict(max_bytes=1)), ([128, 2], dict(max_bytes=8 * 37 * 128, n_trk=37)), ([130], dict(n_trk=37)),
                                 ([64, 64, 2], dict(max_bytes=8 * 37 * 100))):
                res = joint.joint_hazard(scan, slon, slat, levels, anchors=anchors, unit=unit, **kw, **size)
                assert [c[0].size for c in calls] == blocks
                assert np.array_equal(np.concatenate([c[0] for c in calls]), slon[order])          # the sites went in spatial order, once
                del calls[:]
                assert res['joint'].dtype == np.int32 and res['n_set'].dtype == np.int32
                assert np.array_equal(res['joint'], want) and np.array_equal(res['n_set'], want_set)
                assert np.array_equal(res['anchors'], anchors) and np.array_equal(res['levels'], np.asarray(levels))
                assert res['n_unit'] == (37 if unit == 'storm' else 5)
                assert np.array_equal(res['counts'], direct['counts']) and np.array_equal(res['thresholds'], thr)
                results.append(res)
        # every site an anchor: the square in the caller's order, symmetric, with n_set on its diagonal
        full = joint.joint_hazard(scan, slon, slat, levels, max_bytes=1)
        del calls[:]
        want, want_set = JN.joint(m, levels)
        assert np.array_equal(full['joint'], want) and np.array_equal(full['anchors'], np.arange(130))
        assert np.array_equal(full['joint'], full['joint'].transpose(0, 2, 1))
        assert np.array_equal(np.diagonal(full['joint'], axis1=1, axis2=2), want_set)
    # the absolute levels at the scan's thresholds: the diagonal is the scan's own counts summed over groups
    res = joint.joint_hazard(scan, slon, slat, thr, max_bytes=1)
    assert np.array_equal(res['n_set'].T, direct['counts'].sum(axis=1))
    # groups that do not fit the plane are found at the first block
    with pytest.raises(ValueError):
        joint.joint_hazard(scan, slon, slat, [20.0], unit='group', groups=groups[:-1])


def test_pure_functions_by_hand():
    from tropical_cyclone_risk_amd import joint
    j = np.array([[[4, 0, 2], [0, 0, 0]]], np.int32)                        # one level, anchors 0 and 1, three sites
    n_set = np.array([[4, 0, 5]], np.int32)
    anchors = np.array([0, 1])
    rp = joint.joint_return_periods(j, 100)
    assert rp.dtype == np.float64 and rp.tolist() == [[[25.0, np.inf, 50.0], [np.inf, np.inf, np.inf]]]
    c = joint.conditional(j, n_set, anchors)
    assert c[0, 0].tolist() == [1.0, 0.0, 0.5] and np.isnan(c[0, 1]).all() and c.shape == (1, 2, 3)
    e = joint.either(j, n_set, anchors)
    assert e.tolist() == [[[4, 4, 7], [4, 0, 5]]]
    assert joint.conditional(j[:, ::-1], n_set, anchors[::-1])[0, 1].tolist() == [1.0, 0.0, 0.5]


def test_cli_needs_exactly_one_kind_of_level(tmp_path):
    from tropical_cyclone_risk_amd import joint
    a = joint.parse_args(['x.nc', '--site', '1,2', '--thresholds', '33,50'])
    assert a.thresholds.tolist() == [33.0, 50.0] and a.return_periods is None and a.unit == 'storm' and a.anchor == [] and a.out == 'joint.npz'
    a = joint.parse_args(['x.nc', '--site', '1,2', '--anchor=-80,25', '--anchor', '1,2', '--return-periods', '10,50', '--unit', 'year', '--substeps', '2'])
    assert a.return_periods.tolist() == [10.0, 50.0] and a.thresholds is None and a.unit == 'year' and a.anchor == [(-80.0, 25.0), (1.0, 2.0)]
    assert a.substeps == 2
    lon, lat, idx = joint.cli_sites(a)
    assert lon.tolist() == [1.0, -80.0] and lat.tolist() == [2.0, 25.0] and idx.tolist() == [1, 0]         # an anchor not among the sites is added
    csv = tmp_path / 's.csv'
    csv.write_text('lon,lat\n3,4\n5,6\n')
    a = joint.parse_args(['x.nc', '--sites-csv', str(csv), '--thresholds', '33'])
    assert joint.cli_sites(a)[0].tolist() == [3.0, 5.0] and joint.cli_sites(a)[2] is None
    for bad in ([], ['--thresholds', '33', '--return-periods', '10'], ['--thresholds', 'nan'], ['--thresholds', 'x'], ['--thresholds', ''],
                ['--thresholds', ','.join(['1'] * 17)], ['--return-periods', ','.join(['10'] * 17)], ['--thresholds', '33', '--unit', 'month']):
        with pytest.raises(SystemExit):
            joint.parse_args(['x.nc', '--site', '1,2'] + bad)
    with pytest.raises(SystemExit):
        joint.parse_args(['x.nc', '--thresholds', '33'])                       # no sites


# ------------------------------------------------------------------------------------------------------------------ GPU
def _ctx():
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    return L, h


def _rows_of(lev, n_row):
    lev = np.asarray(lev, dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(lev, (n_row, lev.shape[-1])) if lev.ndim == 1 else lev)


def _host_joint(L, h, buf, n_col, lev, unit_of=None, n_unit=None):
    """tcr_joint_host on the [n_row][n_col] view of buf [n_row][row_stride]: (counts [n_level][n_row][n_row], n_set)."""
    n_row = buf.shape[0]
    lev = _rows_of(lev, n_row)
    n_level = lev.shape[1]
    counts, n_set = np.full((n_level, n_row, n_row), -1, np.int32), np.full((n_level, n_row), -1, np.int32)
    u = None if unit_of is None else np.ascontiguousarray(unit_of, dtype=np.int32)
    rc = L.tcr_joint_host(h, buf.ctypes.data, n_row, n_col, buf.shape[1], lev.ctypes.data, n_level, None if u is None else u.ctypes.data,
                          n_col if u is None else n_unit, counts.ctypes.data, n_set.ctypes.data)
    assert rc == 0, L.tcr_last_error(h)
    return counts, n_set


def _both_entry_points(buf, n_col, lev, unit_of=None, n_unit=None):
    """pack_bits on the [n_row][n_col] view of buf [n_row][row_stride] as a tensor (tcr_joint_pack_dev, on a side stream, read where
    it lies) and as a NumPy array, then cross_counts, against the restatement; and tcr_joint_host on the same view.  Returns the
    restatement's (bits, n_set)."""
    import torch
    from tropical_cyclone_risk_amd import joint
    view = buf[:, :n_col]
    want_bits, want_set = JN.pack_bits(view, lev, unit_of, n_unit)
    want_counts = JN.joint(view, lev, None, unit_of, n_unit)[0]
    dev = torch.device('cuda', 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        t = torch.as_tensor(buf, device=dev)[:, :n_col]
        assert t.stride() == (buf.shape[1], 1) or buf.shape[0] == 1
        bits, n_set = joint.pack_bits(t, lev, unit_of, n_unit)
        counts = joint.cross_counts(bits)
        assert bits.dtype == torch.int64 and n_set.dtype == torch.int32 and counts.dtype == torch.int32 and bits.device == t.device
    side.synchronize()
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), want_bits), 'tcr_joint_pack_dev: bits'
    assert np.array_equal(n_set.cpu().numpy(), want_set), 'tcr_joint_pack_dev: n_set'
    assert np.array_equal(counts.cpu().numpy(), want_counts), 'tcr_joint_cross_dev'
    nb, ns = joint.pack_bits(view, lev, unit_of, n_unit)
    assert nb.dtype == np.uint64 and ns.dtype == np.int32 and np.array_equal(nb, want_bits) and np.array_equal(ns, want_set)
    L, h = _ctx()
    try:
        hc, hs = _host_joint(L, h, buf, n_col, lev, unit_of, n_unit)
    finally:
        L.tcr_ctx_destroy(h)
    assert np.array_equal(hc, want_counts) and np.array_equal(hs, want_set), 'tcr_joint_host'
    return want_bits, want_set


def _plane(rng, n_row, n_col, row_stride):
    """Values around the levels 17.5 / 30 / 45 with NaN among them, some exactly on a level; finite decoys above every level in the gap."""
    buf = np.empty((n_row, row_stride))
    v = np.round(rng.normal(30.0, 15.0, (n_row, n_col)), 1)
    v[rng.random(v.shape) < 0.3] = np.nan
    v[rng.random(v.shape) < 0.1] = 17.5
    buf[:, :n_col] = v
    buf[:, n_col:] = 1e9 + rng.random((n_row, row_stride - n_col))
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize('n_level', [1, 3])
@pytest.mark.parametrize('n_col', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_gpu_pack_identity_shapes_with_a_row_stride(built_lib, n_col, n_level):
    rng = np.random.default_rng(300 + n_col)
    buf = _plane(rng, 5, n_col, n_col + 3)
    buf[1, :n_col] = np.nan                                                # a row nothing reaches
    buf[2, :n_col] = 99.0                                                  # and one everything does: the padding bits show
    lev = [17.5, 30.0, 45.0][:n_level] if n_col % 2 else rng.choice([17.5, 30.0, 45.0, -np.inf], (5, n_level))
    bits, n_set = _both_entry_points(buf, n_col, lev)
    n_word = (n_col + 63) // 64
    assert bits.shape == (n_level, 5, n_word) and (n_set[:, 1] == 0).all() and (n_set[:, 2] == n_col).all()
    if n_col % 64:
        assert (bits[:, :, -1] >> np.uint64(n_col % 64) == 0).all()          # nothing at or past n_unit, decoys or not
    pop = np.array([[sum(bin(int(w)).count('1') for w in bits[l, r]) for r in range(5)] for l in range(n_level)])
    assert np.array_equal(pop, n_set)


@pytest.mark.gpu
@pytest.mark.parametrize('n_row', [5, 70000])
def test_gpu_pack_many_short_rows_into_a_larger_table(built_lib, n_row):
    """More rows than the grid cap, packed as a block into a table of more rows: the words round the block stay as they were."""
    import torch
    rng = np.random.default_rng(23)
    plane = np.round(rng.normal(0.0, 3.0, (n_row, 5)), 1)
    plane[rng.random(plane.shape) < 0.3] = np.nan
    lev = np.array([0.0, 2.5])
    want_bits, want_set = JN.pack_bits(plane, lev)
    first, total, guard = 7, n_row + 11, 0x5A5A5A5A5A5A5A5A
    dev = torch.device('cuda', 0)
    table = torch.full((2, total + 2, 1), guard, dtype=torch.int64, device=dev)        # level_stride = total + 2 > total x n_word
    n_set = torch.full((2, n_row + 3), -7, dtype=torch.int32, device=dev)
    tp, tl = torch.as_tensor(plane, device=dev), torch.as_tensor(_rows_of(lev, n_row), device=dev)
    L, h = _ctx()
    try:
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        assert L.tcr_joint_pack_dev(h, tp.data_ptr(), n_row, 5, 5, tl.data_ptr(), 2, None, 5, table.data_ptr() + 8 * first, total + 2,
                                    n_set.data_ptr(), n_row + 3, st) == 0, L.tcr_last_error(h)
        torch.cuda.synchronize()
    finally:
        L.tcr_ctx_destroy(h)
    got = table.cpu().numpy()[:, :, 0]
    assert np.array_equal(got[:, first:first + n_row].view(np.uint64), want_bits[:, :, 0])
    assert (got[:, :first] == guard).all() and (got[:, first + n_row:] == guard).all()
    got_set = n_set.cpu().numpy()
    assert np.array_equal(got_set[:, :n_row], want_set) and (got_set[:, n_row:] == -7).all()
    assert set(np.unique(want_set)) == set(range(6)) or n_row == 5


@pytest.mark.gpu
def test_gpu_pack_special_values_at_every_level(built_lib):
    rng = np.random.default_rng(7)
    n_col = 300
    rows = np.stack([SPECIAL[rng.permutation(np.resize(np.arange(SPECIAL.size), n_col))] for _ in range(3)] + [np.resize(SPECIAL, n_col)])
    levels = [lev for lev, _ in SPECIAL_REACH]
    bits, n_set = _both_entry_points(np.ascontiguousarray(rows), n_col, levels)
    for l, (lev, cols) in enumerate(SPECIAL_REACH):
        assert n_set[l].tolist() == [len(cols) * (n_col // SPECIAL.size)] * 4, lev
        assert int(bits[l, 3, 0]) & 0xFFF == _word(cols), lev
    _both_entry_points(np.ascontiguousarray(rows), n_col, [0.0], rng.integers(0, 7, n_col), 9)          # and through a mapping


@pytest.mark.gpu
@pytest.mark.parametrize('n_unit', [1, 64, 65, 300])
def test_gpu_pack_mapped_units(built_lib, n_unit):
    rng = np.random.default_rng(500 + n_unit)
    n_col = 777
    buf = _plane(rng, 6, n_col, n_col + 3)
    buf[1, :n_col] = np.nan
    buf[2, :n_col] = 99.0
    unit_of = rng.integers(0, n_unit, n_col)
    unit_of[unit_of == n_unit // 2] = 0                                    # an empty unit (where there are two)
    bits, n_set = _both_entry_points(buf, n_col, [17.5, 30.0, 45.0], unit_of, n_unit)
    assert (n_set[:, 2] == np.unique(unit_of).size).all() and (n_set[:, 1] == 0).all()
    if n_unit % 64:
        assert (bits[:, :, -1] >> np.uint64(n_unit % 64) == 0).all()
    one = np.full(n_col, n_unit - 1)                                       # every storm in one unit, the last
    bits, n_set = _both_entry_points(buf, n_col, rng.choice([17.5, 30.0, 45.0], (6, 2)), one, n_unit)
    assert set(np.unique(n_set)) == {0, 1} and n_set[:, 2].tolist() == [1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize('n_unit,n_level', [(130000, 3), (2 ** 18 - 5, 2)])
def test_gpu_pack_mapped_units_in_groups_of_levels(built_lib, n_unit, n_level):
    """More words than the kernel's image holds for all levels at once (4096): two levels and then one, or one at a time."""
    import torch
    from tropical_cyclone_risk_amd import joint
    rng = np.random.default_rng(n_unit)
    n_col = 3000
    plane = _plane(rng, 3, n_col, n_col)
    unit_of = rng.integers(0, n_unit, n_col)
    unit_of[:40] = unit_of[40:80]                                          # units of several storms
    unit_of[-1] = n_unit - 1
    plane[0, -1] = 99.0
    lev = [17.5, 30.0, 45.0][:n_level]
    E = JN.exceed(plane, lev, unit_of, n_unit)
    assert (n_unit + 63) // 64 * n_level > 4096 and E[:, 0, n_unit - 1].all()
    bits, n_set = joint.pack_bits(torch.as_tensor(plane, device=torch.device('cuda', 0)), lev, unit_of, n_unit)
    bits = bits.cpu().numpy().view(np.uint64)
    assert bits.shape == (n_level, 3, (n_unit + 63) // 64)
    assert np.array_equal(JN.unpack(bits, n_unit), E) and np.array_equal(n_set.cpu().numpy(), E.sum(axis=2))
    assert (bits[:, :, -1] >> np.uint64(n_unit % 64) == 0).all()


def _random_bits(rng, shape, density, n_unit):
    """uint64 [shape][n_word] with bits at the density, none at or past n_unit."""
    n_word = (n_unit + 63) // 64
    E = rng.random(tuple(shape) + (64 * n_word,)) < density
    E[..., n_unit:] = False
    return JN.words(E), E


@pytest.mark.gpu
@pytest.mark.parametrize('n_a,n_b', [(1, 1), (63, 65), (64, 64), (65, 130), (130, 1)])
def test_gpu_cross_shapes_words_and_densities(built_lib, n_a, n_b):
    import torch
    from tropical_cyclone_risk_amd import _lib, joint
    kw = _lib.JOINT_KW
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(1000 * n_a + n_b)
    for n_word in (1, kw - 1, kw, kw + 1, 2 * kw + 3):
        n_unit = 64 * n_word - 3
        for density in (0.5, 0.02):
            a, Ea = _random_bits(rng, (3, n_a), density, n_unit)
            b, Eb = _random_bits(rng, (3, n_b), density, n_unit)
            want = JN.cross_from_bool(Ea, Eb)
            assert want.max() > 0 or density < 0.1
            ta, tb = (torch.as_tensor(x.view(np.int64), device=dev) for x in (a, b))
            got = joint.cross_counts(ta, tb)
            assert got.dtype == torch.int32 and tuple(got.shape) == (3, n_a, n_b) and np.array_equal(got.cpu().numpy(), want), (n_word, density)
        assert np.array_equal(joint.cross_counts(a, b), want)              # the NumPy flavour, once per width
        # rows of all ones: every count is n_unit exactly (a lost word or a leaked padding bit would show)
        ones = joint.pack_bits(torch.ones((max(n_a, n_b), n_unit), dtype=torch.float64, device=dev), [0.5, 1.0, 1.0])[0]
        got = joint.cross_counts(ones[:, :n_a], ones[:, :n_b]).cpu().numpy()
        assert (got == n_unit).all() and got.shape == (3, n_a, n_b), n_word


@pytest.mark.gpu
def test_gpu_cross_of_a_table_with_itself_and_of_strided_tables(built_lib):
    import torch
    from tropical_cyclone_risk_amd import _lib, joint
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(77)
    n_col = 64 * _lib.JOINT_KW + 70
    plane = _plane(rng, 150, n_col, n_col)
    lev = [17.5, 30.0, 45.0]
    bits, n_set = joint.pack_bits(torch.as_tensor(plane, device=dev), lev)
    sq = joint.cross_counts(bits).cpu().numpy()
    want, want_set = JN.joint(plane, lev)
    assert np.array_equal(sq, want) and np.array_equal(sq, sq.transpose(0, 2, 1))
    assert np.array_equal(np.diagonal(sq, axis1=1, axis2=2), n_set.cpu().numpy()) and np.array_equal(n_set.cpu().numpy(), want_set)
    # a block of rows of the table (its level stride is the table's) against a table of its own
    a, b = bits[:, 20:97], bits[:, 5:140].contiguous()
    assert a.stride(0) == 150 * bits.shape[2] and b.stride(0) == 135 * bits.shape[2]
    got = joint.cross_counts(a, b).cpu().numpy()
    assert np.array_equal(got, want[:, 20:97, 5:140])
    # rows that are not adjacent are copied first, and the NumPy flavour agrees
    assert np.array_equal(joint.cross_counts(bits[:, ::2], bits).cpu().numpy(), want[:, ::2])
    assert np.array_equal(joint.cross_counts(bits.cpu().numpy().view(np.uint64)[:, 20:97], b.cpu().numpy()), want[:, 20:97, 5:140])


@pytest.mark.gpu
def test_gpu_abi_rejects_bad_arguments_and_a_host_call_that_is_too_large(built_lib):
    import torch
    L, h = _ctx()
    try:
        plane = np.arange(12.0).reshape(3, 4)
        lev = np.array([[5.0, 7.0]] * 3)
        unit = np.array([0, 1, 1, 2], np.int32)
        counts, n_set = np.full((2, 3, 3), -1, np.int32), np.full((2, 3), -1, np.int32)
        p = lambda a: None if a is None else a.ctypes.data                  # noqa: E731

        def call(n_row=3, n_col=4, stride=4, lev_=lev, n_level=2, unit_=None, n_unit=4, counts_=counts, plane_=plane):
            return L.tcr_joint_host(h, p(plane_), n_row, n_col, stride, p(lev_), n_level, p(unit_), n_unit, p(counts_), p(n_set))
        nan_lev = lev.copy()
        nan_lev[2, 1] = np.nan
        for bad in (dict(lev_=nan_lev), dict(stride=3), dict(n_col=0), dict(n_col=2 ** 31), dict(n_row=-1), dict(plane_=None), dict(lev_=None),
                    dict(counts_=None), dict(n_level=0), dict(n_level=17), dict(n_unit=5), dict(unit_=unit, n_unit=2), dict(unit_=unit, n_unit=0),
                    dict(unit_=unit, n_unit=2 ** 18 + 1), dict(unit_=np.array([0, 1, -1, 2], np.int32), n_unit=3)):
            assert call(**bad) == -1, bad
            assert L.tcr_last_error(h).decode().startswith('tcr_joint:'), (bad, L.tcr_last_error(h))
        assert (counts == -1).all() and (n_set == -1).all()                # none of them wrote anything
        assert call() == 0 and n_set.tolist() == [[0, 3, 4], [0, 1, 4]] and counts[0].tolist() == [[0, 0, 0], [0, 3, 3], [0, 3, 4]]
        assert call(unit_=unit, n_unit=3) == 0 and n_set.tolist() == [[0, 2, 3], [0, 1, 3]]
        assert call(n_row=0, plane_=None) == 0
        # over the host entry point's limit: a message, and nothing allocated (the counts alone would be 6.4 GB)
        big, big_lev = np.zeros((40000, 1)), np.zeros((40000, 1))
        assert L.tcr_joint_host(h, big.ctypes.data, 40000, 1, 1, big_lev.ctypes.data, 1, None, 1, counts.ctypes.data, None) == -1
        msg = L.tcr_last_error(h).decode()
        assert msg.startswith('tcr_joint:') and 'too large for tcr_joint_host' in msg, msg
        # the _dev entry points
        dev = torch.device('cuda', 0)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        tp, tl = torch.as_tensor(plane, device=dev), torch.as_tensor(lev, device=dev)
        tb = torch.full((2, 3, 1), -1, dtype=torch.int64, device=dev)
        ts = torch.full((2, 3), -1, dtype=torch.int32, device=dev)
        tc = torch.full((2, 3, 3), -1, dtype=torch.int32, device=dev)
        tu = torch.as_tensor(unit, device=dev)

        def pack(n_row=3, n_col=4, stride=4, n_level=2, unit_=None, n_unit=4, level_stride=3, set_stride=3, bits_=tb.data_ptr()):
            return L.tcr_joint_pack_dev(h, tp.data_ptr(), n_row, n_col, stride, tl.data_ptr(), n_level, unit_, n_unit, bits_, level_stride,
                                        ts.data_ptr(), set_stride, st)
        for bad in (dict(stride=3), dict(n_col=0), dict(n_level=0), dict(n_level=17), dict(n_unit=3), dict(level_stride=2), dict(set_stride=2),
                    dict(bits_=None), dict(unit_=tu.data_ptr(), n_unit=2 ** 18 + 1), dict(n_row=-1)):
            assert pack(**bad) == -1, bad
            assert L.tcr_last_error(h).decode().startswith('tcr_joint:'), (bad, L.tcr_last_error(h))

        def cross(n_a=3, n_b=3, sa=3, sb=3, n_word=1, n_level=2, a_=tb.data_ptr(), c_=tc.data_ptr()):
            return L.tcr_joint_cross_dev(h, a_, n_a, sa, tb.data_ptr(), n_b, sb, n_word, n_level, c_, st)
        for bad in (dict(n_a=-1), dict(n_b=-1), dict(sa=2), dict(sb=2), dict(n_word=-1), dict(n_level=0), dict(n_level=17), dict(a_=None),
                    dict(c_=None), dict(n_a=65536 * 64)):
            assert cross(**bad) == -1, bad
            assert L.tcr_last_error(h).decode().startswith('tcr_joint:'), (bad, L.tcr_last_error(h))
        torch.cuda.synchronize()
        assert (tb.cpu() == -1).all() and (ts.cpu() == -1).all() and (tc.cpu() == -1).all()
        # a unit out of range cannot be reported by the _dev entry point: that column sets no bit
        tu2 = torch.as_tensor(np.array([0, 7, -1, 2], np.int32), device=dev)
        assert pack(unit_=tu2.data_ptr(), n_unit=3) == 0 and cross() == 0
        torch.cuda.synchronize()
        assert tb.cpu().numpy()[:, :, 0].tolist() == [[0, 0b100, 0b101], [0, 0b100, 0b101]] and ts.cpu().tolist() == [[0, 1, 2], [0, 1, 2]]
        assert tc.cpu().numpy()[1].tolist() == [[0, 0, 0], [0, 1, 1], [0, 1, 2]]
    finally:
        L.tcr_ctx_destroy(h)


def _small_ensemble(rng, n_trk=40, n_t=30, n_site=150):
    """The ensemble shape of test_levels._small_ensemble: random walks in one box, hourly, some with NaN tails; sites in and around
    the box, three far away; 10 groups (years)."""
    lon = rng.uniform(280, 300, (n_trk, 1)) + np.cumsum(rng.normal(-0.1, 0.15, (n_trk, n_t)), axis=1)
    lat = rng.uniform(15, 35, (n_trk, 1)) + np.cumsum(rng.normal(0.08, 0.1, (n_trk, n_t)), axis=1)
    v = np.clip(30 + np.cumsum(rng.normal(0.2, 1.5, (n_trk, n_t)), axis=1), 12, 80)
    env = [rng.normal(0, 6, (n_trk, n_t)) for _ in range(4)]
    end = rng.integers(4, n_t + 1, n_trk)
    for p in [lon, lat, v] + env:
        p[np.arange(n_t)[None, :] >= end[:, None]] = np.nan
    slon, slat = rng.uniform(276, 302, n_site), rng.uniform(12, 40, n_site)
    slon[[3, 77, 149]], slat[[3, 77, 149]] = [100.0, 20.0, -170.0], [-30.0, 60.0, 5.0]          # no storm reaches these
    return lon, lat, v, env, rng.integers(0, 10, n_trk), slon, slat


@pytest.mark.gpu
def test_gpu_joint_hazard_of_the_wind_footprint_against_its_own_plane_and_counts(built_lib):
    import torch
    from tropical_cyclone_risk_amd import joint, levels, windfield
    from tropical_cyclone_risk_amd.analysis import to_numpy
    lon, lat, v, env, groups, slon, slat = _small_ensemble(np.random.default_rng(31))
    dev = torch.device('cuda', 0)
    put = lambda x: torch.as_tensor(x, device=dev)                          # noqa: E731
    thr = np.arange(10.0, 71.0, 5.0)
    lev = thr[[0, 2, 4]]
    sizes = []

    def scan_of(tracks, g):
        tl, ta, tv, tenv = tracks

        def scan(x, y):
            sizes.append(int(x.shape[0]))
            return windfield.site_wind(tl, ta, tv, tenv, g, x, y, 3600.0, thresholds=thr, return_max=True, n_groups=10)
        return scan
    scan = scan_of((put(lon), put(lat), put(v), [put(e) for e in env]), groups)
    sl, sa = put(slon), put(slat)
    direct = scan(sl, sa)
    m, counts = to_numpy(direct['site_max']), to_numpy(direct['counts'])
    del sizes[:]
    reached = (~np.isnan(m)).sum(axis=1)
    anchors = np.concatenate([np.argsort(-reached, kind='stable')[:1], [3], np.argsort(-reached, kind='stable')[1:3]])     # site 3: no storm
    res = {}
    for unit, kw, map_ in (('storm', {}, {}), ('group', dict(groups=groups, n_groups=10), dict(unit_of=groups, n_unit=10))):
        want, want_set = JN.joint(m, lev, anchors, **map_)
        assert want.sum() > 30 and (want[:, 1] == 0).all()
        blocked = joint.joint_hazard(scan, sl, sa, lev, anchors=anchors, unit=unit, max_bytes=1, **kw)
        one = joint.joint_hazard(scan, sl, sa, lev, anchors=anchors, unit=unit, n_trk=40, **kw)
        assert sizes == [64, 64, 22, 150]
        del sizes[:]
        for r in (blocked, one):
            assert r['joint'].device == sl.device and r['joint'].dtype == torch.int32 and r['n_unit'] == (40 if unit == 'storm' else 10)
            assert np.array_equal(to_numpy(r['joint']), want) and np.array_equal(to_numpy(r['n_set']), want_set)
            assert np.array_equal(to_numpy(r['counts']), counts) and np.array_equal(to_numpy(r['thresholds']), thr)
        res[unit] = want, want_set
    # the diagonal at the scan's own thresholds is the scan's counts summed over groups
    full = joint.joint_hazard(scan, sl, sa, lev, max_bytes=1)
    sq, n_set = to_numpy(full['joint']), to_numpy(full['n_set'])
    assert np.array_equal(np.diagonal(sq, axis1=1, axis2=2), n_set) and np.array_equal(n_set.T, counts.sum(axis=1)[:, [0, 2, 4]])
    assert np.array_equal(sq, JN.joint(m, lev)[0]) and np.array_equal(sq[:, anchors], res['storm'][0])
    # a permutation of the sites permutes the result
    perm = np.random.default_rng(5).permutation(150)
    inv = np.argsort(perm)
    r = joint.joint_hazard(scan, put(slon[perm]), put(slat[perm]), lev, anchors=inv[anchors], max_bytes=1)
    assert np.array_equal(to_numpy(r['joint'])[:, :, inv], res['storm'][0]) and np.array_equal(to_numpy(r['n_set'])[:, inv], res['storm'][1])
    # a permutation of the storms leaves the counts per storm as they are
    sp = np.random.default_rng(6).permutation(40)
    scan_p = scan_of((put(lon[sp]), put(lat[sp]), put(v[sp]), [put(e[sp]) for e in env]), groups[sp])
    r = joint.joint_hazard(scan_p, sl, sa, lev, anchors=anchors, max_bytes=1)
    assert np.array_equal(to_numpy(r['joint']), res['storm'][0]) and np.array_equal(to_numpy(r['n_set']), res['storm'][1])
    # every site's own return levels as its levels: at least k storms reach the k-th largest value (ties can add)
    T = np.array([5.0, 10.0])
    k, defined = levels.ranks_of_periods(T, 10)
    rl = to_numpy(levels.site_return_levels(scan, sl, sa, 10, T, max_bytes=1)['return_level'])
    own = np.where(np.isnan(rl), np.inf, rl)
    r = joint.joint_hazard(scan, sl, sa, own, anchors=anchors, max_bytes=1)
    n_set = to_numpy(r['n_set'])
    assert defined.all() and k.tolist() == [2, 1] and (~np.isnan(rl)).sum() > 50 and np.isnan(rl).any()
    for l in range(2):
        ok = ~np.isnan(rl[:, l])
        assert (n_set[l][ok] >= k[l]).all() and (n_set[l][~ok] == 0).all()
    assert np.array_equal(to_numpy(r['joint']), JN.joint(m, own, anchors)[0])


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
    nl = _nl(output_directory=str(tmp_path), exp_name='jt', start_year=2001, end_year=2003)
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
    from tropical_cyclone_risk_amd import analysis, joint, levels, windfield
    fn = _write_track_file(tmp_path, np.random.default_rng(5))
    sites = ['--site=-75.0,24.0', '--site', '286.5,25.5', '--site=-72.25,27.0', '--site', '10.0,50.0']
    lon, lat, vmax, v, env, groups, gfile, gyear, dt = analysis.load_wind_planes([fn])
    assert lon.shape[0] == 13
    slon, slat = np.array([-75.0, 286.5, -72.25, 10.0, 287.0]), np.array([24.0, 25.5, 27.0, 50.0, 26.0])
    m = windfield.site_wind(lon, lat, v, env, groups, slon, slat, dt, return_max=True, n_groups=3)['site_max']
    keys = {'joint', 'n_set', 'anchors', 'levels', 'n_unit', 'unit', 'joint_return_period', 'conditional', 'counts', 'thresholds', 'site_lon',
            'site_lat', 'total_years', 'r_out_km', 'substeps', 'rmax_km', 'dt_s', 'group_file', 'group_year', 'files'}
    # absolute levels, per storm: the anchor 287,26 is not among the sites and becomes the fifth; 286.5,25.5 is the second
    out = str(tmp_path / 'a.npz')
    assert joint.main([fn, '--out', out, '--thresholds', '12.5,20', '--anchor', '287.0,26.0', '--anchor', '286.5,25.5'] + sites) == 0
    text = capsys.readouterr().out
    assert 'P(site | anchor)' in text and '5 sites' in text
    z = np.load(out)
    assert set(z.files) == keys and z['anchors'].tolist() == [4, 1] and np.array_equal(z['site_lon'], slon) and z['n_unit'] == 13
    want, want_set = JN.joint(m, [12.5, 20.0], [4, 1])
    assert want.sum() >= 3 and np.array_equal(z['joint'], want) and np.array_equal(z['n_set'], want_set) and str(z['unit']) == 'storm'
    assert np.array_equal(z['joint_return_period'], joint.joint_return_periods(want, 3))
    # every site's own return levels, per year, all pairs
    out = str(tmp_path / 'b.npz')
    assert joint.main([fn, '--out', out, '--return-periods', '1,3', '--unit', 'year'] + sites) == 0
    text = capsys.readouterr().out
    assert 'sites have no level' in text
    z = np.load(out)
    assert set(z.files) == keys | {'return_periods', 'return_level'} and z['anchors'].tolist() == [0, 1, 2, 3] and z['n_unit'] == 3
    rl = z['return_level']
    assert np.isnan(rl[3]).all() and np.array_equal(z['levels'], np.where(np.isnan(rl), np.inf, rl))
    want, want_set = JN.joint(m[:4], z['levels'], None, groups, 3)
    assert np.array_equal(z['joint'], want) and np.array_equal(z['n_set'], want_set) and want.sum() >= 1
    k = levels.ranks_of_periods([1.0, 3.0], 3)[0]
    assert k.tolist() == [3, 1]
