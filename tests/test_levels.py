"""Return levels (tropical_cyclone_risk_amd/levels.py, csrc/tcr_select.hip): the k-th largest value of every row of a per-storm
plane that is not NaN, and the blocked pass that turns a site analysis into the N-year wind or rain at every site.  CPU tests pin
the NumPy restatement (tests/levels_numpy.py) and the rank rule to hand values, and check the argument handling and the blocked
driver on a scan made of NumPy; GPU tests (`-m gpu`) check the kernel against the restatement on both of its paths, and the levels
against the counts of the scan they come from.  Nothing here has a tolerance: every comparison is of bits, NaN equal to NaN."""
import ctypes
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import levels_numpy as LN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_NAN = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]        # a NaN with the sign bit set (and a payload)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_by_hand():
    assert np.isnan(NEG_NAN) and np.signbit(NEG_NAN)
    row = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3.5, -3.5, NEG_NAN, 1e-310, -1e-310])
    k = LN.keys(row[~np.isnan(row)])
    assert k.dtype == np.uint64 and LN.same_bits(LN.values(k), row[~np.isnan(row)])
    assert LN.keys([0.0])[0] == 1 << 63 and LN.keys([-0.0])[0] == (1 << 63) - 1
    assert LN.keys([-np.inf])[0] == 0x000FFFFFFFFFFFFF and LN.keys([np.inf])[0] == 0xFFF0000000000000
    want = [np.inf, 3.5, 1e-310, 0.0, -0.0, -1e-310, -3.5, -np.inf]                # descending: +0.0 before -0.0
    level, n_valid = LN.row_select(row[None, :], [1, 2, 3, 4, 5, 6, 7, 8, 9, 4])
    assert n_valid.tolist() == [8]
    assert LN.same_bits(level[0, :8], want) and np.isnan(level[0, 8]) and LN.same_bits(level[0, 9], 0.0)
    assert not np.signbit(level[0, 3]) and np.signbit(level[0, 4])
    # a row of NaNs of both signs, and ties
    level, n_valid = LN.row_select(np.array([[np.nan, NEG_NAN, np.nan], [2.0, 2.0, 1.0]]), [1, 2, 3, 4])
    assert n_valid.tolist() == [0, 3] and np.isnan(level[0]).all()
    assert LN.same_bits(level[1], [2.0, 2.0, 1.0, np.nan])
    assert not LN.same_bits([0.0], [-0.0]) and LN.same_bits([np.nan], [NEG_NAN])
    # as many ranks as a call may carry, in descending order of rank: the row backwards, then NaN
    from tropical_cyclone_risk_amd import _lib
    ranks = np.arange(_lib.SELECT_MAX_RANKS, 0, -1)
    level, _ = LN.row_select(np.arange(40.0)[None, :], ranks)
    assert LN.same_bits(level[0, -40:], np.arange(40.0)) and np.isnan(level[0, :-40]).all() and level.shape == (1, 64)


def test_ranks_of_periods_by_hand():
    from tropical_cyclone_risk_amd import levels, loss
    from tests import loss_numpy
    k, ok = levels.ranks_of_periods([10.0, 45.0, 46.0, 0.5], 45)
    assert k.dtype == np.int64 and k.tolist()[:2] == [5, 1] and k[3] == 90 and ok.tolist() == [True, True, False, True]
    # where the rounding of the division puts ceil(Y / T) off by one, in either direction
    for Y, T, naive, want in ((45, 45.0 / 39.0, 39, 40), (100, 100.0 / 29.0, 30, 29)):
        assert int(np.ceil(Y / T)) == naive
        k, ok = levels.ranks_of_periods([T], Y)
        assert k.tolist() == [want] and ok.all()
        assert want * T >= Y and (want - 1) * T < Y                    # the smallest integer with k T >= Y, in the arithmetic used
    for bad in ([0.0], [-1.0], [np.nan], [np.inf], [10.0, 0.0]):
        with pytest.raises(ValueError):
            levels.ranks_of_periods(bad, 45)
    with pytest.raises(ValueError):
        levels.ranks_of_periods([10.0], 0)
    # the loss curves are built on the same rule and have not moved
    assert loss.DEFAULT_RETURN_PERIODS == levels.DEFAULT_RETURN_PERIODS == (10.0, 25.0, 50.0, 100.0, 250.0)
    rng = np.random.default_rng(2)
    y = rng.gamma(2.0, 3.0, 100)
    T = np.concatenate([[1.0, 100.0, 101.0, 0.3, 100.0 / 29.0, 0.6211180124223602], rng.uniform(0.5, 120.0, 40)])
    assert LN.same_bits(loss.loss_curve(y, 100, T), loss_numpy.loss_curve(y, 100, T))


def test_select_symbols_exported_constants_and_abi_version_unchanged(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_select_dev', 'tcr_select_host'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    L.tcr_abi_version.restype = ctypes.c_int
    assert L.tcr_abi_version() == 7 and _lib.TCR_ABI_VERSION == 7
    src = '#include <stdio.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%d %d\\n",TCR_SELECT_LDS_KEYS,TCR_SELECT_MAX_RANKS);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'k.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'k')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        assert [int(x) for x in subprocess.check_output([exe]).split()] == [_lib.SELECT_LDS_KEYS, _lib.SELECT_MAX_RANKS]
    assert _lib.SELECT_MAX_RANKS == 64 and _lib.SELECT_LDS_KEYS >= 1024


def test_argument_errors_before_any_device_work(monkeypatch):
    from tropical_cyclone_risk_amd import _lib, levels

    def no_library():
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', no_library)
    plane = np.arange(12.0).reshape(3, 4)
    for ranks in ([0], [1, -2], [], np.ones(65, np.int64), [1.5], [[1, 2]], [True], np.array([1.0])):
        with pytest.raises(ValueError):
            levels.row_select(plane, ranks)
    for bad in (np.arange(4.0), np.zeros((3, 0)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            levels.row_select(bad, [1])
    with pytest.raises(AssertionError, match='the library was touched'):
        levels.row_select(plane, [1, 4, 5])

    def scan(x, y):
        raise AssertionError('the scan was called before the arguments were checked')
    lon, lat = np.array([280.0, 281.0]), np.array([20.0, 21.0])
    for kw in (dict(return_periods=[0.0]), dict(return_periods=[np.nan]), dict(return_periods=[]), dict(return_periods=np.arange(1.0, 66.0)),
               dict(total_years=0), dict(max_bytes=0), dict(site_lat=lat[:1]), dict(site_lat=np.array([np.nan, 1.0])),
               dict(site_lon=np.array([]), site_lat=np.array([]))):
        with pytest.raises(ValueError):
            levels.site_return_levels(**dict(dict(scan=scan, site_lon=lon, site_lat=lat, total_years=10, return_periods=[2.0]), **kw))
    with pytest.raises(AssertionError, match='the scan was called'):
        levels.site_return_levels(scan, lon, lat, 10, [2.0])


def _fake_scan(rng, n_trk=37, n_groups=4):
    """A site analysis made of NumPy: storm s is a disc of radius r_s degrees around (cx_s, cy_s) with peak p_s, and a site's
    value of it falls off with the distance (NaN outside).  A site's row depends on that site alone, as in the real scans."""
    cx, cy, rad, peak = rng.uniform(270, 300, n_trk), rng.uniform(10, 40, n_trk), rng.uniform(2, 12, n_trk), rng.uniform(15, 80, n_trk)
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
    return scan, plane, calls, thr


def test_blocked_driver_equals_the_unblocked_one_in_the_callers_site_order(monkeypatch):
    from tropical_cyclone_risk_amd import levels
    from tropical_cyclone_risk_amd.sitescan import spatial_order
    monkeypatch.setattr(levels, 'row_select', lambda plane, ranks, return_valid=False, **kw: LN.row_select(plane, ranks))
    rng = np.random.default_rng(11)
    scan, plane, calls, thr = _fake_scan(rng)
    slon, slat = rng.uniform(268, 302, 130), rng.uniform(8, 42, 130)
    slon[17], slat[17] = 100.0, -30.0                                  # no storm reaches this one
    T = [1.0, 2.5, 5.0, 10.0, 12.0]
    k, ok = levels.ranks_of_periods(T, 10)
    assert k.tolist() == [10, 4, 2, 1, 1] and ok.tolist() == [True] * 4 + [False]
    blocked = levels.site_return_levels(scan, slon, slat, 10, T, max_bytes=1)
    assert [c[0].size for c in calls] == [64, 64, 2]                   # 130 sites: the last block is ragged
    order = spatial_order(slon, slat, np)
    assert np.array_equal(np.concatenate([c[0] for c in calls]), slon[order])          # the sites went in spatial order, once
    assert np.array_equal(np.concatenate([c[1] for c in calls]), slat[order])
    del calls[:]
    one = levels.site_return_levels(scan, slon, slat, 10, T, n_trk=37)
    assert [c[0].size for c in calls] == [130]
    del calls[:]
    probe = levels.site_return_levels(scan, slon, slat, 10, T, max_bytes=8 * 37 * 100)       # n_trk unknown: 64 sites, then 64 more
    assert [c[0].size for c in calls] == [64, 64, 2]
    # the expected result, in the caller's order, without the driver
    m = plane(slon, slat)
    want, n_reach = LN.row_select(m, k)
    want[:, ~ok] = np.nan
    direct = scan(slon, slat)
    assert (~np.isnan(m)).any(axis=1).sum() > 100 and np.isnan(m).all(axis=1).any() and (n_reach >= 4).sum() > 30
    for res in (blocked, one, probe):
        assert LN.same_bits(res['return_level'], want) and res['return_level'].shape == (130, 5)
        assert res['n_reach'].dtype == np.int32 and np.array_equal(res['n_reach'], n_reach)
        assert res['counts'].dtype == np.int32 and np.array_equal(res['counts'], direct['counts'])
        assert np.array_equal(res['thresholds'], thr) and np.array_equal(res['return_periods'], T)
        assert np.isnan(res['return_level'][:, 4]).all() and not np.isnan(res['return_level'][:, 3]).all()
        assert set(res) == {'return_level', 'n_reach', 'counts', 'thresholds', 'return_periods'}
    # levels against counts, with no tolerance: level_k >= thr_b exactly when at least k storms reach thr_b
    c = direct['counts'].sum(axis=1)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(want[:, :4, None] >= thr[None, None, :], c[:, None, :] >= k[None, :4, None])


def test_cli_option_is_off_by_default():
    from tropical_cyclone_risk_amd import hazard, rainfall, windfield
    for mod in (hazard, windfield, rainfall):
        assert mod.parse_args(['x.nc', '--site', '1,2']).return_periods is None
        a = mod.parse_args(['x.nc', '--site', '1,2', '--return-periods', '10,50,2.5'])
        assert np.array_equal(a.return_periods, [10.0, 50.0, 2.5])
        for bad in ('0', '10,x', '-5', ''):
            with pytest.raises(SystemExit):
                mod.parse_args(['x.nc', '--site', '1,2', '--return-periods', bad])


# ------------------------------------------------------------------------------------------------------------------ GPU
def _both_entry_points(buf, n_col, ranks):
    """row_select on the [n_row][n_col] view of buf [n_row][row_stride] through tcr_select_host (NumPy) and tcr_select_dev (torch);
    the view is read where it lies: the columns past n_col are never selected."""
    import torch
    from tropical_cyclone_risk_amd import levels
    want = LN.row_select(buf[:, :n_col], ranks)
    view = buf[:, :n_col]
    assert not view.flags['C_CONTIGUOUS'] or buf.shape[1] == n_col
    lv, nv = levels.row_select(view, ranks, return_valid=True)
    assert LN.same_bits(lv, want[0]), 'tcr_select_host'
    assert nv.dtype == np.int32 and np.array_equal(nv, want[1])
    t = torch.as_tensor(buf, device=torch.device('cuda', 0))[:, :n_col]
    assert t.stride() == (buf.shape[1], 1)
    tl, tv = levels.row_select(t, ranks, return_valid=True)
    assert tl.device == t.device and tv.dtype == torch.int32
    assert LN.same_bits(tl.cpu().numpy(), want[0]), 'tcr_select_dev'
    assert np.array_equal(tv.cpu().numpy(), want[1])
    assert LN.same_bits(levels.row_select(t, ranks).cpu().numpy(), want[0])            # without n_valid
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('n_col', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_gpu_shapes_with_a_row_stride(built_lib, n_col):
    rng = np.random.default_rng(100 + n_col)
    n_row = 6
    buf = rng.normal(0.0, 40.0, (n_row, n_col + 3))
    buf[:, n_col:] = 1e9 + rng.random((n_row, 3))                          # finite decoys in the gap: larger than every value
    hole = rng.random((n_row, n_col)) < 0.5
    hole[0] = False if n_col == 1 else hole[0]
    buf[:, :n_col][hole] = np.nan
    count = int((~hole[0]).sum())
    ranks = [1, 2, max(count, 1), count + 1, n_col, 2]
    level, n_valid = _both_entry_points(buf, n_col, ranks)
    assert n_valid[0] == count and not np.isnan(level[0, 2]) and np.isnan(level[0, 3])
    assert (level[~np.isnan(level)] < 1e8).all()


@pytest.mark.gpu
def test_gpu_values_that_break_a_radix_pass_or_the_key_map(built_lib):
    rng = np.random.default_rng(7)
    n_col = 300
    one = np.full(n_col, np.nan)
    one[123] = -7.25
    four = rng.permutation(np.resize(np.array([3.0, -3.0, 1e-3, 2.5e7]), n_col))
    mixed = rng.permutation(np.resize(np.array([np.inf, -np.inf, 0.0, -0.0, 1.5, -1.5, np.nan, NEG_NAN, 5e-324, -5e-324, 1e300, -1e300]), n_col))
    sub = rng.permutation(np.concatenate([np.arange(1, 141) * 5e-324, -np.arange(1, 141) * 5e-324, [0.0, -0.0] * 10]))
    base = np.array([37.123], dtype=np.float64).view(np.uint64)[0]
    low_bit = (base + rng.integers(0, 2, n_col).astype(np.uint64)).view(np.float64)          # x and the next double after x
    top_exp = rng.permutation(np.resize(np.ldexp(1.25, [-1000, -512, -1, 0, 1, 512, 1000]), n_col))
    top_exp[::7] *= -1.0
    rows = np.stack([np.full(n_col, np.nan), one, np.full(n_col, 41.5), four, mixed, sub, low_bit, top_exp])
    rows[0, ::2] = NEG_NAN
    assert sub.size == n_col and np.unique(low_bit).size == 2 and rows.shape == (8, n_col)
    ranks = [1, 2, 3, 4, 5, 75, 76, 150, 151, 226, 250, 251, 299, 300, 301, 150]
    level, n_valid = _both_entry_points(np.ascontiguousarray(rows), n_col, ranks)
    assert n_valid.tolist() == [0, 1, 300, 300, 250, 300, 300, 300]
    assert np.isnan(level[0]).all() and LN.same_bits(level[1, :2], [-7.25, np.nan]) and LN.same_bits(level[2, :14], np.full(14, 41.5))
    assert LN.same_bits(level[3, [4, 5, 6, 7, 8, 9]], [2.5e7, 2.5e7, 3.0, 3.0, 1e-3, -3.0])
    assert LN.same_bits(level[4, 0], np.inf) and LN.same_bits(level[4, 10], -np.inf) and np.isnan(level[4, 11])


@pytest.mark.gpu
def test_gpu_both_sides_of_the_lds_boundary(built_lib):
    """Rows with C - 1, C and C + 1 values that are not NaN (C keys fit in LDS; one more and the row is selected from global
    memory), a row without a NaN, and permuted copies of the rows at C and C + 1: another order of the values in LDS, the same
    result."""
    from tropical_cyclone_risk_amd import _lib
    rng = np.random.default_rng(19)
    C = _lib.SELECT_LDS_KEYS
    n_col = 2 * C + 5
    vals = np.where(rng.random((4, n_col)) < 0.5, np.round(rng.normal(30.0, 20.0, (4, n_col)), 1), rng.normal(0.0, 1e3, (4, n_col)))
    for r, keep in enumerate((C - 1, C, C + 1)):
        vals[r, rng.permutation(n_col)[keep:]] = np.nan
    rows = np.concatenate([vals, vals[1:3, rng.permutation(n_col)]])
    ranks = [1, C, C + 1, n_col, n_col + 1]
    level, n_valid = _both_entry_points(np.ascontiguousarray(rows), n_col, ranks)
    assert n_valid.tolist() == [C - 1, C, C + 1, n_col, C, C + 1]
    assert np.isnan(level[0, 1]) and not np.isnan(level[1, 1]) and np.isnan(level[1, 2]) and not np.isnan(level[2, 2])
    assert not np.isnan(level[3, 3]) and np.isnan(level[:, 4]).all()
    assert LN.same_bits(level[4], level[1]) and LN.same_bits(level[5], level[2])


@pytest.mark.gpu
def test_gpu_many_short_rows(built_lib):
    import torch
    from tropical_cyclone_risk_amd import levels
    rng = np.random.default_rng(23)
    plane = np.round(rng.normal(0.0, 3.0, (70000, 8)), 1)                   # ties, and both zeros
    plane[rng.random(plane.shape) < 0.5] = np.nan
    plane[plane == 0.0] *= rng.choice([1.0, -1.0], (plane == 0.0).sum())
    ranks = [1, 2, 3, 5, 8, 9]
    want, n_valid = LN.row_select(plane, ranks)
    got, nv = levels.row_select(torch.as_tensor(plane, device=torch.device('cuda', 0)), ranks, return_valid=True)
    assert LN.same_bits(got.cpu().numpy(), want) and np.array_equal(nv.cpu().numpy(), n_valid)
    assert set(np.unique(n_valid)) == set(range(9))


def _small_ensemble(rng, n_trk=40, n_t=30):
    """Random walks in one box, hourly, some with NaN tails; 130 sites in and around the box, three far away; 10 groups (years)."""
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


def _check_levels_of_a_scan(scan, plane_key, slon, slat, n_trk, thr):
    """site_return_levels in 64-site blocks and in one block: identical, the restatement applied to the scan's own plane, and tied
    to the scan's own counts without a tolerance."""
    from tropical_cyclone_risk_amd import levels
    from tropical_cyclone_risk_amd.analysis import to_numpy
    T = [1.0, 2.0, 5.0, 10.0, 20.0]
    k, ok = levels.ranks_of_periods(T, 10)
    assert k.tolist() == [10, 5, 2, 1, 1] and ok.tolist() == [True] * 4 + [False]
    sizes = []

    def counted(x, y):
        sizes.append(int(x.shape[0]))
        return scan(x, y)
    blocked = {n: to_numpy(a) for n, a in levels.site_return_levels(counted, slon, slat, 10, T, key=plane_key, max_bytes=1).items()}
    assert sizes == [64, 64, 2]
    del sizes[:]
    one = {n: to_numpy(a) for n, a in levels.site_return_levels(counted, slon, slat, 10, T, key=plane_key, n_trk=n_trk).items()}
    assert sizes == [130]
    direct = scan(slon, slat)
    m, counts = to_numpy(direct[plane_key]), to_numpy(direct['counts'])
    want, n_reach = LN.row_select(m, k)
    want[:, ~ok] = np.nan
    assert (n_reach >= 10).sum() >= 5 and (n_reach == 0).sum() >= 1, np.bincount(n_reach)
    for res in (blocked, one):
        assert LN.same_bits(res['return_level'], want)
        assert np.array_equal(res['n_reach'], n_reach) and np.array_equal(res['n_reach'], (~np.isnan(m)).sum(axis=1))
        assert np.array_equal(res['counts'], counts) and np.array_equal(res['thresholds'], thr)
    c = counts.sum(axis=1)
    assert (c[:, 0] >= 5).any() and (c[:, -1] == 0).any() and (c > 0).sum() > 200
    with np.errstate(invalid='ignore'):
        assert np.array_equal(want[:, :4, None] >= thr[None, None, :], c[:, None, :] >= k[None, :4, None])


@pytest.mark.gpu
def test_gpu_levels_of_the_wind_footprint_against_its_own_counts(built_lib):
    import torch
    from tropical_cyclone_risk_amd import windfield
    lon, lat, v, env, groups, slon, slat = _small_ensemble(np.random.default_rng(31))
    dev = torch.device('cuda', 0)
    tl, ta, tv, sl, sa = (torch.as_tensor(x, device=dev) for x in (lon, lat, v, slon, slat))
    tenv = [torch.as_tensor(x, device=dev) for x in env]
    thr = np.arange(10.0, 71.0, 5.0)

    def scan(x, y):
        return windfield.site_wind(tl, ta, tv, tenv, groups, x, y, 3600.0, thresholds=thr, return_max=True, n_groups=10)
    _check_levels_of_a_scan(scan, 'site_max', sl, sa, lon.shape[0], thr)


@pytest.mark.gpu
@pytest.mark.parametrize('stat', ['total', 'peak-rate'])
def test_gpu_levels_of_the_rainfall_against_its_own_counts(built_lib, stat):
    """The NumPy flavour: every block crosses to the device and back through the _host entry points."""
    from tropical_cyclone_risk_amd import rainfall
    lon, lat, v, env, groups, slon, slat = _small_ensemble(np.random.default_rng(37))
    thr = np.array([1.0, 5.0, 10.0, 25.0, 50.0, 100.0, 200.0]) if stat == 'total' else np.array([0.5, 1.0, 2.0, 4.0, 8.0, 12.0])

    def scan(x, y):
        return rainfall.site_rain(lon, lat, v, groups, x, y, 3600.0, stat=stat, thresholds=thr, return_values=True, n_groups=10)
    _check_levels_of_a_scan(scan, rainfall.STATS[stat][1], slon, slat, lon.shape[0], thr)


@pytest.mark.gpu
def test_gpu_abi_rejects_bad_arguments(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        plane = np.arange(12.0).reshape(3, 4)
        level = np.full((3, 2), -1.0)
        valid = np.full(3, -1, np.int32)

        def call(n_row=3, n_col=4, stride=4, ranks=(1, 4), n_rank=None, plane_=plane, level_=level):
            r = (ctypes.c_int64 * max(len(ranks), 1))(*ranks)
            return L.tcr_select_host(h, None if plane_ is None else plane_.ctypes.data, n_row, n_col, stride,
                                     len(ranks) if n_rank is None else n_rank, r, None if level_ is None else level_.ctypes.data,
                                     valid.ctypes.data)
        for p in (dict(n_row=-1), dict(n_col=0), dict(n_col=2 ** 31), dict(stride=3), dict(ranks=(0,)), dict(ranks=(2, -1)), dict(n_rank=0),
                  dict(n_rank=65), dict(plane_=None), dict(level_=None)):
            assert call(**p) == -1, p
            assert L.tcr_last_error(h).decode().startswith('tcr_select:'), (p, L.tcr_last_error(h))
        assert (level == -1.0).all() and (valid == -1).all()                 # none of them wrote anything
        assert call(n_row=0) == 0 and (level == -1.0).all()
        assert call() == 0
        assert level.tolist() == [[3.0, 0.0], [7.0, 4.0], [11.0, 8.0]] and valid.tolist() == [4, 4, 4]
    finally:
        L.tcr_ctx_destroy(h)


def _nl(**over):
    from tropical_cyclone_risk_amd import namelist
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    for k, val in over.items():
        setattr(nl, k, val)
    return nl


def _write_track_file(tmp_path, rng):
    """Three years with 6, 0 and 7 storms in one file written by io.write_tracks, on the namelist's time axis."""
    from tropical_cyclone_risk_amd import io as tio
    from tropical_cyclone_risk_amd.basins import TC_Basin
    nl = _nl(output_directory=str(tmp_path), exp_name='lv', start_year=2001, end_year=2003)
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
    """--return-periods adds return_level, return_periods and n_reach to the .npz of hazard, windfield and rainfall and leaves the
    other keys as they are; without the option the keys are those of before."""
    from tropical_cyclone_risk_amd import analysis, hazard, levels, rainfall, windfield
    fn = _write_track_file(tmp_path, np.random.default_rng(5))
    sites0 = ['--site=-75.0,24.0', '--site', '286.5,25.5', '--site=-72.25,27.0', '--site', '10.0,50.0']
    base = {'counts', 'return_period', 'thresholds', 'site_lon', 'site_lat', 'total_years', 'group_file', 'group_year', 'files'}
    before = {hazard: base | {'radius_km'}, windfield: base | {'r_out_km', 'substeps', 'rmax_km', 'dt_s'},
              rainfall: base | {'r_out_km', 'substeps', 'stat', 'dt_s'}}
    lon, lat, vmax, v, env, groups, gfile, gyear, dt = analysis.load_wind_planes([fn])
    k, ok = levels.ranks_of_periods([2.0, 5.0], 3)
    assert k.tolist() == [2, 1] and ok.tolist() == [True, False] and lon.shape[0] == 13
    for mod, key, more, call in (
            (hazard, 'site_max', ['--radius-km', '400'],
             lambda x, y: hazard.site_hazard(lon, lat, vmax, groups, x, y, radius_km=400.0, return_max=True, n_groups=3)),
            (windfield, 'site_max', [],
             lambda x, y: windfield.site_wind(lon, lat, v, env, groups, x, y, dt, return_max=True, n_groups=3)),
            (rainfall, 'site_total', [],
             lambda x, y: rainfall.site_rain(lon, lat, vmax, groups, x, y, dt, return_values=True, n_groups=3))):
        out = str(tmp_path / (mod.__name__.split('.')[-1] + '.npz'))
        sites = sites0 + more
        assert mod.main([fn, '--out', out] + sites) == 0
        plain = np.load(out)
        assert set(plain.files) == before[mod], mod.__name__
        text = capsys.readouterr().out
        assert 'return period' in text and 'return level' not in text
        assert mod.main([fn, '--out', out, '--return-periods', '2,5'] + sites) == 0
        z = np.load(out)
        assert set(z.files) == before[mod] | {'return_level', 'return_periods', 'n_reach'}, mod.__name__
        text = capsys.readouterr().out
        assert 'return period' in text and 'return level' in text
        for name in before[mod]:
            same = (z[name] == plain[name]) | ((z[name] != z[name]) & (plain[name] != plain[name]))
            assert np.all(same), (mod.__name__, name)
        api = call(z['site_lon'], z['site_lat'])
        want, n_reach = LN.row_select(api[key], k)
        want[:, ~ok] = np.nan
        assert np.array_equal(z['return_periods'], [2.0, 5.0]) and z['return_level'].shape == (4, 2)
        assert LN.same_bits(z['return_level'], want) and np.array_equal(z['n_reach'], n_reach) and z['n_reach'].dtype == np.int32
        assert n_reach[3] == 0 and (n_reach[:3] >= 2).all() and not np.isnan(want[:3, 0]).any()
