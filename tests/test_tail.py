"""Tail-fitted return levels (tropical_cyclone_risk_amd/levels.py row_tail, csrc/tcr_tail.hip): a generalized Pareto distribution
fitted to the excesses of every row's k largest values over its (k+1)-th, and the levels of return periods past the record.  CPU
tests pin the NumPy restatement (tests/tail_numpy.py) to hand values, the order of its sums, the estimators, the argument handling
and the blocked driver on a scan made of NumPy; GPU tests (`-m gpu`) check the kernel against the restatement through both entry
points.  threshold, xi, sigma and n_valid are compared as bits, NaN equal to NaN.  The levels go through log and expm1 and are
held to |gpu - ref| <= 1e-13 (|u| + |ref - u|): both sides' log and expm1 are within a few ulp, expm1 amplifies a relative error
of its argument by at most 1 + |xi L| <= 23 here (k T / total_years <= 1e7 and xi <= 1; for xi L < 0 by less than 1), so tens of
ulp are expected and 1e-13 is about 900."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import levels_numpy as LN
from tests import tail_numpy as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_NAN = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]        # a NaN with the sign bit set (and a payload)
LEVEL_TOL = 1e-13
KEYS = ('threshold', 'xi', 'sigma', 'level', 'n_valid')


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_by_hand():
    T = [100.0]
    # one value above a threshold that the other three tie with: S1 = 0, a1 = 0, no fit
    r = TN.row_tail([[4.0, 3.0, 3.0, 3.0, 3.0, 1.0, np.nan]], 4, 10, T)
    n, u, y = TN.excesses([4.0, 3.0, 3.0, 3.0, 3.0, 1.0, np.nan], 4)
    assert (n, u, y.tolist()) == (6, 3.0, [0.0, 0.0, 0.0, 1.0]) and not np.signbit(y).any()
    assert r['n_valid'].tolist() == [6] and r['threshold'].tolist() == [3.0]
    assert np.isnan(r['xi'][0]) and np.isnan(r['sigma'][0]) and np.isnan(r['level']).all()
    # excesses all zero
    r = TN.row_tail([[3.0, 3.0, 3.0, 3.0, 3.0, 1.0]], 4, 10, T)
    assert TN.excesses([3.0, 3.0, 3.0, 3.0, 3.0, 1.0], 4)[2].tolist() == [0.0] * 4
    assert r['threshold'].tolist() == [3.0] and np.isnan(r['xi'][0]) and np.isnan(r['level']).all()
    # n_valid = k: no threshold; n_valid = k + 1: a fit
    r = TN.row_tail([[5.0, 1.0, 2.0, 4.0, np.nan, NEG_NAN], [5.0, 1.0, 2.0, 4.0, 0.5, np.nan]], 4, 10, T)
    assert r['n_valid'].tolist() == [4, 5] and np.isnan(r['threshold'][0]) and r['threshold'][1] == 0.5
    assert np.isnan([r['xi'][0], r['sigma'][0], r['level'][0, 0]]).all()
    assert not np.isnan([r['xi'][1], r['sigma'][1], r['level'][1, 0]]).any()
    # k = 2, y = [1, 3]: a0 = 2, a1 = 1/2, d = 1, xi = 0 exactly, sigma = 2: the xi == 0 branch.  L < 0 is NaN for that period only
    r = TN.row_tail([[13.0, 10.0, 11.0]], 2, 10, [100.0, 5.0, 4.0])
    assert r['threshold'].tolist() == [10.0] and r['xi'].tolist() == [0.0] and r['sigma'].tolist() == [2.0]
    L = TN.log_periods(2, 10, [100.0, 5.0, 4.0])
    assert L[0] == np.log(20.0) and L[1] == 0.0 and L[2] < 0
    assert r['level'][0, 0] == 10.0 + 2.0 * L[0] and r['level'][0, 1] == 10.0 and np.isnan(r['level'][0, 2])
    # k = 3, y = [1, 2, 6]: S0 = 9, S1 = 2 * 1 + 1 * 2 = 4, a0 = 3, a1 = 2/3, d = 5/3, xi = 2 - 9/5 = 0.2, sigma = 2 * 3 * (2/3) / (5/3) = 2.4
    r = TN.row_tail([[2.0, 7.0, 1.0, 3.0, -4.0]], 3, 6, [20.0])
    assert r['threshold'].tolist() == [1.0] and abs(r['xi'][0] - 0.2) < 1e-15 and abs(r['sigma'][0] - 2.4) < 1e-15
    assert abs(r['level'][0, 0] - (1.0 + 2.4 * (10.0 ** 0.2 - 1.0) / 0.2)) < 1e-13
    # an infinity among the excesses fails the fit by itself; the threshold is still the row's own
    r = TN.row_tail([[np.inf, 7.0, 1.0, 3.0, -4.0], [2.0, 7.0, -np.inf, 3.0, -np.inf]], 3, 6, [20.0])
    assert r['threshold'].tolist() == [1.0, -np.inf] and np.isnan(r['xi']).all() and np.isnan(r['level']).all()
    # -0.0 and +0.0 are two values, in that order; a tie at the threshold has excess +0.0
    n, u, y = TN.excesses([0.0, -0.0, 1.0, -0.0], 2)
    assert n == 4 and np.signbit(u) and u == 0.0 and y.tolist() == [0.0, 1.0] and not np.signbit(y[0])


def _explicit_pairing(v):
    """The tree by halves: the sum of a block of 2^m entries is the sum of its left half plus the sum of its right half."""
    if len(v) == 1:
        return v[0]
    return _explicit_pairing(v[:len(v) // 2]) + _explicit_pairing(v[len(v) // 2:])


def test_tree_sum_is_the_stated_pairing_and_no_other_order():
    rng = np.random.default_rng(3)
    for k in (2, 3, 37, 256):
        v = rng.gamma(0.5, 10.0, k) * 10.0 ** rng.integers(-6, 7, k)
        P = max(2, 1 << (k - 1).bit_length())
        padded = [float(x) for x in v] + [0.0] * (P - k)
        assert len(padded) in (2, 4, 64, 256) and TN.tree_sum(v) == _explicit_pairing(padded)
    assert TN.tree_sum([1.0, 2.0, 3.0]) == 6.0 and TN.tree_sum([5.0]) == 5.0
    # (1 + e) + (e + e) = 1 + 2^-52 with e = 2^-53, where adding one e at a time never leaves 1
    v = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53])
    seq = 0.0
    for x in v:
        seq += float(x)
    assert TN.tree_sum(v) == 1.0 + 2.0 ** -52 and seq == 1.0 and float(np.sum(v)) == 1.0
    assert TN.tree_sum(v) != seq and TN.tree_sum(v) != float(np.sum(v))


@pytest.mark.parametrize('xi, want', [(-0.25, -0.2419), (0.15, 0.1513)])
def test_estimators_recover_exact_quantiles(xi, want):
    k, sigma = 256, 10.0
    q = (np.arange(1, k + 1) - 0.5) / k
    y = sigma * ((1.0 - q) ** (-xi) - 1.0) / xi
    row = np.concatenate([[50.0], 50.0 + y])
    r = TN.row_tail(row[None, ::-1], k, 45, [1000.0])
    assert r['threshold'][0] == 50.0 and abs(r['xi'][0] - xi) < 0.01 and abs(r['xi'][0] - want) < 5e-5
    assert abs(r['sigma'][0] / sigma - 1.0) < 0.02
    assert r['xi'][0] <= 1.0


def test_tail_symbols_exported_constant_and_abi_version_unchanged(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_tail_dev', 'tcr_tail_host'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    L.tcr_abi_version.restype = ctypes.c_int
    assert L.tcr_abi_version() == 7 and _lib.TCR_ABI_VERSION == 7
    src = '#include <stdio.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%d\\n",TCR_TAIL_MAX_K);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'k.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'k')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        assert int(subprocess.check_output([exe])) == _lib.TAIL_MAX_K == 2048


def test_argument_errors_before_any_device_work(monkeypatch):
    from tropical_cyclone_risk_amd import _lib, hazard, levels, rainfall, windfield

    def no_library():
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', no_library)
    plane = np.arange(12.0).reshape(3, 4)
    for k in (1, 2049, 2.5, True, 0, -3, '4', None, np.float64(4.0)):
        with pytest.raises(ValueError):
            levels.row_tail(plane, k, 10, [100.0])
    for years in (0, np.nan, -1.0, np.inf, 'x'):
        with pytest.raises(ValueError):
            levels.row_tail(plane, 2, years, [100.0])
    for periods in ([0.0], [-1.0], [np.nan], [np.inf], [10.0, 0.0], [], np.arange(1.0, 66.0), [[1.0, 2.0]], 5.0, ['x']):
        with pytest.raises(ValueError):
            levels.row_tail(plane, 2, 10, periods)
    for bad in (np.arange(4.0), np.zeros((3, 0)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            levels.row_tail(bad, 2, 10, [100.0])
    with pytest.raises(AssertionError, match='the library was touched'):
        levels.row_tail(plane, np.int32(2), 10.5, [100.0, 1000.0])

    def scan(x, y):
        raise AssertionError('the scan was called before the arguments were checked')
    lon, lat = np.array([280.0, 281.0]), np.array([20.0, 21.0])
    for k in (1, 2049, 2.5, True):
        with pytest.raises(ValueError):
            levels.site_return_levels(scan, lon, lat, 10, [2.0], tail_exceedances=k)
    with pytest.raises(AssertionError, match='the scan was called'):
        levels.site_return_levels(scan, lon, lat, 10, [2.0], tail_exceedances=2)
    # the command lines: the option needs --return-periods, and an integer in range
    for mod in (hazard, windfield, rainfall):
        base = ['x.nc', '--site', '1,2']
        assert mod.parse_args(base).tail_exceedances is None
        assert mod.parse_args(base + ['--return-periods', '100,1000']).tail_exceedances is None
        assert mod.parse_args(base + ['--return-periods', '100,1000', '--tail-exceedances', '256']).tail_exceedances == 256
        with pytest.raises(SystemExit):
            mod.parse_args(base + ['--tail-exceedances', '256'])
        for bad in ('1', '2049', '2.5', 'x', ''):
            with pytest.raises(SystemExit):
                mod.parse_args(base + ['--return-periods', '100', '--tail-exceedances', bad])


def test_blocked_driver_with_the_tail_in_the_callers_site_order(monkeypatch):
    from tests.test_levels import _fake_scan
    from tropical_cyclone_risk_amd import levels
    monkeypatch.setattr(levels, 'row_select', lambda plane, ranks, return_valid=False, **kw: LN.row_select(plane, ranks))
    monkeypatch.setattr(levels, 'row_tail', lambda plane, k, total_years, periods, **kw: TN.row_tail(plane, k, total_years, periods))
    rng = np.random.default_rng(11)
    scan, plane, calls, thr = _fake_scan(rng)
    slon, slat = rng.uniform(268, 302, 130), rng.uniform(8, 42, 130)
    slon[17], slat[17] = 100.0, -30.0                                  # no storm reaches this one
    T = [1.0, 5.0, 10.0, 100.0, 1000.0]
    today = {'return_level', 'n_reach', 'counts', 'thresholds', 'return_periods'}
    plain = levels.site_return_levels(scan, slon, slat, 10, T, max_bytes=1)
    assert set(plain) == today
    assert set(levels.site_return_levels(scan, slon, slat, 10, T, max_bytes=1, tail_exceedances=None)) == today
    del calls[:]
    blocked = levels.site_return_levels(scan, slon, slat, 10, T, max_bytes=1, tail_exceedances=3)
    assert [c[0].size for c in calls] == [64, 64, 2]
    del calls[:]
    one = levels.site_return_levels(scan, slon, slat, 10, T, n_trk=37, tail_exceedances=3)
    assert [c[0].size for c in calls] == [130]
    want = TN.row_tail(plane(slon, slat), 3, 10, T)                    # in the caller's order, without the driver
    fitted = ~np.isnan(want['xi'])
    assert fitted.sum() > 30 and (want['n_valid'] < 4).sum() > 5 and want['n_valid'][17] == 0
    for res in (blocked, one):
        assert set(res) == today | set(levels.TAIL_KEYS) == today | {'tail_level', 'tail_xi', 'tail_sigma', 'tail_threshold'}
        assert res['tail_level'].shape == (130, 5) and res['tail_xi'].shape == (130,)
        for name, ref in (('tail_level', 'level'), ('tail_xi', 'xi'), ('tail_sigma', 'sigma'), ('tail_threshold', 'threshold')):
            assert LN.same_bits(res[name], want[ref]), name
        for name in ('return_level', 'n_reach', 'counts'):                 # unchanged by the tail
            assert LN.same_bits(res[name], plain[name]) and res[name].dtype == plain[name].dtype, name
        # past the record the order statistic has nothing to say and the fit has
        assert np.isnan(res['return_level'][:, 3:]).all() and not np.isnan(res['tail_level'][fitted][:, 3:]).any()
        assert np.isnan(res['tail_level'][:, 0]).all()                      # L = log(3 / 10) < 0
        assert np.array_equal(res['n_reach'], want['n_valid'])
    assert set(levels.npz_keys(one)) == {'return_level', 'return_periods', 'n_reach'} | set(levels.TAIL_KEYS)
    assert set(levels.npz_keys(plain)) == {'return_level', 'return_periods', 'n_reach'}


# ------------------------------------------------------------------------------------------------------------------ GPU
def _level_error(got, want):
    """max over the levels of |gpu - ref| / (|u| + |ref - u|) (0 where both are NaN); a level that is NaN on one side only fails."""
    g, w, u = got['level'], want['level'], want['threshold'][:, None]
    assert np.array_equal(np.isnan(g), np.isnan(w)), 'a level is NaN on one side only'
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.abs(g - w) / (np.abs(u) + np.abs(w - u))
    rel[np.isnan(w) | (g == w)] = 0.0
    return float(rel.max()) if rel.size else 0.0


def _compare(got, want, what):
    for name in ('threshold', 'xi', 'sigma'):
        assert LN.same_bits(got[name], want[name]), (what, name)
    assert got['n_valid'].dtype == np.int32 and np.array_equal(got['n_valid'], want['n_valid']), what
    assert got['level'].shape == want['level'].shape
    err = _level_error(got, want)
    print('%s: max |gpu - ref| / (|u| + |ref - u|) over the levels = %.3g' % (what, err))
    assert err <= LEVEL_TOL, (what, err)
    return err


def _both_entry_points(buf, n_col, k, total_years, T, want=None):
    """row_tail on the [n_row][n_col] view of buf [n_row][row_stride] through tcr_tail_host (NumPy) and tcr_tail_dev (torch), the
    view read where it lies, against the restatement; the threshold against row_select's (k+1)-th largest, bit for bit."""
    import torch
    from tropical_cyclone_risk_amd import levels
    from tropical_cyclone_risk_amd.analysis import to_numpy
    view = buf[:, :n_col]
    want = TN.row_tail(view, k, total_years, T) if want is None else want
    assert not view.flags['C_CONTIGUOUS'] or buf.shape[1] == n_col
    got = levels.row_tail(view, k, total_years, T)
    assert set(got) == set(KEYS) and all(isinstance(got[n], np.ndarray) for n in KEYS)
    _compare(got, want, 'tcr_tail_host k=%d' % k)
    t = torch.as_tensor(buf, device=torch.device('cuda', 0))[:, :n_col]
    assert t.stride() == (buf.shape[1], 1)
    dev = levels.row_tail(t, k, total_years, T)
    assert all(dev[n].device == t.device for n in KEYS) and dev['n_valid'].dtype == torch.int32
    _compare({n: to_numpy(dev[n]) for n in KEYS}, want, 'tcr_tail_dev k=%d' % k)
    assert LN.same_bits(to_numpy(levels.row_select(t, [k + 1]))[:, 0], want['threshold']), 'threshold != row_select(k + 1)'
    return want


def _fill(rng, n, scale=8.0):
    """n heavy-tailed positive values with ties (rounded), like storm peaks at a site."""
    return np.round(15.0 + scale * rng.pareto(6.0, n) * 5.0, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('k', [2, 3, 37, 256, 2048])
def test_gpu_rows_that_decide_a_step_of_the_definition(built_lib, k):
    rng = np.random.default_rng(500 + k)
    n_col = 2 * k + 37
    rows = []

    def row(values):
        v = np.full(n_col, np.nan)
        v[1::2] = NEG_NAN                                                      # NaNs of both signs around the values
        values = np.asarray(values, dtype=np.float64)
        v[rng.permutation(n_col)[:values.size]] = values
        rows.append(v)
    for n_valid in (0, k, k + 1, k + 2):
        row(_fill(rng, n_valid))
    row(_fill(rng, n_col))                                                     # no NaN at all
    row(rng.gamma(2.0, 12.0, n_col - 5))                                       # no ties
    row(np.concatenate([_fill(rng, k - 1) + 100.0, np.full(7, 60.0), _fill(rng, 5)]))           # more values at u than needed
    row(np.concatenate([_fill(rng, k - 1) + 100.0, np.full(2, 60.0), _fill(rng, 5)]))           # exactly enough: one tie and u
    row(np.concatenate([np.full(k, 44.5), _fill(rng, 9)]))                     # the top k all equal, above u: d is 0 or a rounding error
    row(np.concatenate([np.full(k + 1, 44.5), _fill(rng, 9)]))                 # the top k and u all equal: every excess +0.0
    row(-_fill(rng, k + 20))                                                   # negatives only
    row(np.concatenate([rng.normal(0.0, 1.0, k), [0.0, -0.0] * 9, -_fill(rng, 3)]))             # u among the zeros of both signs
    row(np.concatenate([[0.0] * 3, [-0.0] * 3, -_fill(rng, k)])[:k + 9])       # the zeros in the top k
    row(np.concatenate([[np.inf], _fill(rng, k + 4)]))                         # +inf in the top k: no fit
    row(np.concatenate([_fill(rng, k), [-np.inf] * 3]))                        # u = -inf: no fit
    row(_fill(rng, k + 30) * 1e-307)                                          # tiny values: subnormal excesses
    buf = np.full((len(rows), n_col + 3), 1e9)                                 # finite decoys in the gap: larger than every value
    buf[:, :n_col] = np.stack(rows)
    T = [0.01, 1.0, 10.0, 100.0, 1000.0, 45.0 / k]                             # the last: L = 0 up to a rounding; k T / Y <= 45 512
    want = _both_entry_points(buf, n_col, k, 45, T)
    assert want['n_valid'][:6].tolist() == [0, k, k + 1, k + 2, n_col, n_col - 5]
    assert np.isnan(want['threshold'][:2]).all() and not np.isnan(want['threshold'][2:]).any()
    fit = ~np.isnan(want['xi'])
    assert fit[[2, 3, 4, 5, 10, 15]].all() and not fit[[0, 1, 9, 13, 14]].any()
    assert fit[[6, 7, 11, 12]].all() or k < 37              # (with two or three exceedances the ties leave a single positive excess)
    assert want['threshold'][6] == 60.0 and want['threshold'][7] == 60.0 and want['threshold'][13] < 1e8
    assert LN.same_bits(want['threshold'][9], 44.5) and want['threshold'][14] == -np.inf
    assert np.isnan(want['level'][:, 0]).all() and not np.isnan(want['level'][fit][:, 1 if k > 45 else 3:5]).any()
    assert (want['xi'][fit] <= 1.0).all() and (want['sigma'][fit][:-1] > 0).all() and want['sigma'][15] >= 0      # (a0 a1 underflows there)


@pytest.mark.gpu
def test_gpu_both_sides_of_the_lds_boundary(built_lib):
    """n_col = 9000: rows with at most and with more than TCR_SELECT_LDS_KEYS values that are not NaN, so the select and the gather
    run from LDS and from the row, and permuted copies of a row of each kind: the same fit, whatever the order of the values."""
    from tropical_cyclone_risk_amd import _lib
    rng = np.random.default_rng(29)
    C, n_col = _lib.SELECT_LDS_KEYS, 9000
    vals = np.stack([_fill(rng, n_col) for _ in range(6)])
    for r, keep in enumerate((300, C - 1, C, C + 1, 8600)):
        vals[r, rng.permutation(n_col)[keep:]] = np.nan
    vals[2, np.argsort(np.nan_to_num(vals[2], nan=-1.0))[-3:]] = 555.5         # ties above u on the LDS path ...
    vals[3, np.argsort(np.nan_to_num(vals[3], nan=-1.0))[-3:]] = 555.5         # ... and on the global path
    rows = np.ascontiguousarray(np.concatenate([vals, vals[2:4, rng.permutation(n_col)]]))
    for k in (256, 2048):
        want = _both_entry_points(rows, n_col, k, 45, [100.0, 250.0, 1000.0, 10000.0])
        assert want['n_valid'].tolist() == [300, C - 1, C, C + 1, 8600, n_col, C, C + 1]
        assert (want['n_valid'] > C).sum() == 4 and (want['n_valid'] <= C).sum() == 4           # both paths ran
        assert not np.isnan(want['xi'][1:]).any() and np.isnan(want['xi'][0]) == (k > 299)
        for name in KEYS:
            assert LN.same_bits(want[name][6], want[name][2]) and LN.same_bits(want[name][7], want[name][3]), name


@pytest.mark.gpu
def test_gpu_more_rows_than_workgroups(built_lib):
    """65 537 rows of 8 values with k = 2: the grid is 65 536 workgroups and the last row goes round.  The rows repeat 257 distinct
    ones, and 65 536 = 255 * 257 + 1, so the row that goes round differs from the row its workgroup had first."""
    import torch
    from tropical_cyclone_risk_amd import levels
    from tropical_cyclone_risk_amd.analysis import to_numpy
    rng = np.random.default_rng(41)
    base = np.round(rng.gamma(2.0, 10.0, (257, 8)), 1)
    base[rng.random(base.shape) < 0.35] = np.nan
    idx = np.arange(65537) % 257
    plane = np.ascontiguousarray(base[idx])
    small = TN.row_tail(base, 2, 45, [100.0, 1000.0])
    want = {n: small[n][idx] for n in KEYS}
    assert set(np.unique(small['n_valid'])) >= {2, 3, 4, 8} and not LN.same_bits(small['level'][0], small['level'][1])
    _compare(levels.row_tail(plane, 2, 45, [100.0, 1000.0]), want, 'tcr_tail_host 65537 rows')
    dev = levels.row_tail(torch.as_tensor(plane, device=torch.device('cuda', 0)), 2, 45, [100.0, 1000.0])
    _compare({n: to_numpy(dev[n]) for n in KEYS}, want, 'tcr_tail_dev 65537 rows')


@pytest.mark.gpu
def test_gpu_blocked_pass_over_the_wind_footprint(built_lib):
    """site_return_levels with the tail over windfield.site_wind at 200 sites: 64-site blocks equal one block bit for bit in every
    key, the keys of before equal the call without the tail, and the tail is the restatement's on the footprint's own plane."""
    import torch
    from tests.test_levels import _small_ensemble
    from tropical_cyclone_risk_amd import levels, windfield
    from tropical_cyclone_risk_amd.analysis import to_numpy
    rng = np.random.default_rng(31)
    lon, lat, v, env, groups, slon, slat = _small_ensemble(rng)
    slon, slat = np.concatenate([slon, rng.uniform(278, 300, 70)]), np.concatenate([slat, rng.uniform(14, 38, 70)])
    dev = torch.device('cuda', 0)
    tl, ta, tv, sl, sa = (torch.as_tensor(x, device=dev) for x in (lon, lat, v, slon, slat))
    tenv = [torch.as_tensor(x, device=dev) for x in env]
    thr = np.arange(10.0, 71.0, 5.0)
    sizes = []

    def scan(x, y):
        sizes.append(int(x.shape[0]))
        return windfield.site_wind(tl, ta, tv, tenv, groups, x, y, 3600.0, thresholds=thr, return_max=True, n_groups=10)
    T = [2.0, 5.0, 10.0, 100.0, 1000.0]
    blocked = {n: to_numpy(a) for n, a in levels.site_return_levels(scan, sl, sa, 10, T, max_bytes=1, tail_exceedances=8).items()}
    assert sizes == [64, 64, 64, 8]
    del sizes[:]
    one = {n: to_numpy(a) for n, a in levels.site_return_levels(scan, sl, sa, 10, T, n_trk=40, tail_exceedances=8).items()}
    assert sizes == [200]
    plain = {n: to_numpy(a) for n, a in levels.site_return_levels(scan, sl, sa, 10, T, n_trk=40).items()}
    assert set(plain) == {'return_level', 'n_reach', 'counts', 'thresholds', 'return_periods'}
    assert set(one) == set(blocked) == set(plain) | set(levels.TAIL_KEYS)
    for name in one:
        assert LN.same_bits(blocked[name], one[name]) and blocked[name].dtype == one[name].dtype, name
    for name in plain:
        assert LN.same_bits(one[name], plain[name]) and one[name].dtype == plain[name].dtype, name
    want = TN.row_tail(to_numpy(scan(sl, sa)['site_max']), 8, 10, T)
    got = dict(threshold=one['tail_threshold'], xi=one['tail_xi'], sigma=one['tail_sigma'], level=one['tail_level'], n_valid=one['n_reach'])
    _compare(got, want, 'site_return_levels over site_wind')
    fit = ~np.isnan(want['xi'])
    assert fit.sum() >= 20 and (want['n_valid'] < 9).sum() >= 3
    assert np.isnan(one['return_level'][:, 3:]).all() and not np.isnan(one['tail_level'][fit][:, 1:]).any()


@pytest.mark.gpu
def test_gpu_abi_rejects_bad_arguments(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        plane = np.array([[13.0, 10.0, 11.0, np.nan], [1.0, 2.0, 6.0, 0.0], [np.nan, 1.0, np.nan, 2.0]])
        param = np.full((3, 3), -1.0)
        level = np.full((3, 2), -1.0)
        valid = np.full(3, -1, np.int32)

        def call(n_row=3, n_col=4, stride=4, k=2, years=10.0, periods=(100.0, 4.0), n_period=None, plane_=plane, param_=param, level_=level,
                 periods_null=False):
            T = (ctypes.c_double * max(len(periods), 1))(*periods)
            return L.tcr_tail_host(h, None if plane_ is None else plane_.ctypes.data, n_row, n_col, stride, k, years,
                                   len(periods) if n_period is None else n_period, None if periods_null else T,
                                   None if param_ is None else param_.ctypes.data, None if level_ is None else level_.ctypes.data,
                                   valid.ctypes.data)
        for p in (dict(n_row=-1), dict(n_col=0), dict(n_col=2 ** 31), dict(stride=3), dict(k=1), dict(k=2049), dict(k=0), dict(years=0.0),
                  dict(years=float('nan')), dict(years=float('inf')), dict(years=-2.0), dict(periods=(0.0,)), dict(periods=(10.0, float('nan'))),
                  dict(periods=(float('inf'),)), dict(n_period=0), dict(n_period=65), dict(plane_=None), dict(param_=None), dict(level_=None),
                  dict(periods_null=True)):
            assert call(**p) == -1, p
            assert L.tcr_last_error(h).decode().startswith('tcr_tail:'), (p, L.tcr_last_error(h))
        assert (param == -1.0).all() and (level == -1.0).all() and (valid == -1).all()          # none of them wrote anything
        assert call(n_row=0) == 0 and (level == -1.0).all()
        assert call() == 0
        # row 0: u = 10, y = [1, 3], xi = 0, sigma = 2; row 1: u = 1, y = [1, 5]: a0 = 3, a1 = 1/2, d = 2, xi = 1/2, sigma = 3/2
        assert valid.tolist() == [3, 4, 2] and param[0].tolist() == [10.0, 0.0, 2.0] and param[1].tolist() == [1.0, 0.5, 1.5]
        assert np.isnan(param[2]).all() and np.isnan(level[2]).all() and np.isnan(level[:, 1]).all()
        assert abs(level[0, 0] - (10.0 + 2.0 * np.log(20.0))) < 1e-13 and abs(level[1, 0] - (1.0 + 1.5 * (np.sqrt(20.0) - 1.0) / 0.5)) < 1e-13
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_cli_round_trip(built_lib, tmp_path, capsys):
    """--tail-exceedances adds tail_level, tail_xi, tail_sigma and tail_threshold to the .npz of hazard, windfield and rainfall and
    leaves every other key as --return-periods alone writes it."""
    from tests.test_levels import _write_track_file
    from tropical_cyclone_risk_amd import analysis, hazard, levels, rainfall, windfield
    fn = _write_track_file(tmp_path, np.random.default_rng(5))
    sites = ['--site=-75.0,24.0', '--site', '286.5,25.5', '--site=-72.25,27.0', '--site', '10.0,50.0']
    lon, lat, vmax, v, env, groups, gfile, gyear, dt = analysis.load_wind_planes([fn])
    for mod, key, more, call in (
            (hazard, 'site_max', ['--radius-km', '400'],
             lambda x, y: hazard.site_hazard(lon, lat, vmax, groups, x, y, radius_km=400.0, return_max=True, n_groups=3)),
            (windfield, 'site_max', [],
             lambda x, y: windfield.site_wind(lon, lat, v, env, groups, x, y, dt, return_max=True, n_groups=3)),
            (rainfall, 'site_total', [],
             lambda x, y: rainfall.site_rain(lon, lat, vmax, groups, x, y, dt, return_values=True, n_groups=3))):
        out = str(tmp_path / (mod.__name__.split('.')[-1] + '.npz'))
        assert mod.main([fn, '--out', out, '--return-periods', '2,30'] + sites + more) == 0
        before = dict(np.load(out))
        assert 'fitted tail level' not in capsys.readouterr().out
        assert mod.main([fn, '--out', out, '--return-periods', '2,30', '--tail-exceedances', '4'] + sites + more) == 0
        z = np.load(out)
        assert set(z.files) == set(before) | set(levels.TAIL_KEYS), mod.__name__
        assert 'fitted tail level' in capsys.readouterr().out
        for name in before:
            same = (z[name] == before[name]) | ((z[name] != z[name]) & (before[name] != before[name]))
            assert np.all(same), (mod.__name__, name)
        want = TN.row_tail(call(z['site_lon'], z['site_lat'])[key], 4, 3, [2.0, 30.0])
        got = dict(threshold=z['tail_threshold'], xi=z['tail_xi'], sigma=z['tail_sigma'], level=z['tail_level'], n_valid=z['n_reach'])
        _compare(got, want, mod.__name__)
        assert want['n_valid'][3] == 0 and (want['n_valid'][:3] >= 5).all() and z['tail_level'].shape == (4, 2)
        assert np.isnan(z['return_level'][:, 1]).all() and not np.isnan(z['tail_level'][:3, 1]).all()
