"""Rain accumulation windows (include/tcrisk_hip.h "rain accumulation windows", tropical_cyclone_risk_amd/accumulation.py,
csrc/tcr_accumulation.hip): the largest rain depth of every storm at every site in any m consecutive sample intervals.  CPU tests
pin the NumPy restatement (tests/accumulation_numpy.py) to hand values, to the storm total, to its bounds and to a closed form,
and check the argument handling; GPU tests (`-m gpu`) check the kernel against the restatement on random storms and on hand-made
tracks that take every catch-up path of the mode, its consistency with the rainfall footprint, bit-identity, the entry points and
the command line."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import accumulation_numpy as AN
from tests import levels_numpy as LN
from tests import rainfall_numpy as RN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DT = 3600.0
THR = np.array([5.0, 10.0, 25.0, 50.0, 75.0, 100.0, 150.0, 200.0, 300.0])                 # mm
STRESS_WINDOWS = [1, 3, 6, 24, 47, 96]      # the shortest, one equal to n - 1 = 47, one longer than every track


# ------------------------------------------------------------------------------------------------------------------ CPU
def _km_track(x_km, vmax=40.0, n_t=None):
    """One storm on the equator at x_km kilometres east of 200 E, sample by sample; NaN tail up to n_t samples."""
    x = np.asarray(x_km, float)
    n_t = x.size if n_t is None else n_t
    lon = np.full((1, n_t), np.nan)
    lon[0, :x.size] = 200.0 + np.rad2deg(x / RN.EARTH_R_KM)
    tail = np.isnan(lon)
    return lon, np.where(tail, np.nan, 0.0), np.where(tail, np.nan, vmax)


def _site_km(x_km, lat=0.0):
    return np.array([200.0 + np.rad2deg(x_km / RN.EARTH_R_KM)]), np.array([lat])


def test_restatement_by_hand():
    lon, lat, v = np.array([[280.0, 280.2, 280.4]]), np.array([[20.0, 20.1, 20.2]]), np.array([[30.0, 32.0, 36.0]])
    slon, slat = np.array([280.1]), np.array([20.3])
    for sub in (1, 2):
        rec = RN.records(lon, lat, v, DT, sub)[0]
        nr = 2 * sub + 1
        assert rec.shape == (4, nr)
        hh = DT / 3600.0 / sub / 2
        assert AN.half_step(DT, sub) == hh
        # scalar arithmetic, record by record
        rho = [float(RN.rate(float(RN.haversine_km(rec[0][q], rec[1][q], slon[0], slat[0])), rec[2][q])) for q in range(nr)]
        assert min(rho) > 0
        I = [hh * (rho[q] + rho[q + 1]) for q in range(nr - 1)]
        T = [0.0]
        for k in (1, 2):
            t = T[-1]
            for q in range((k - 1) * sub, k * sub):
                t = t + I[q]
            T.append(t)
        inside, rho_, I_, T_, _ = AN.series(rec, slon, slat, 500.0, DT, sub)
        assert inside.all() and np.allclose(rho_[0], rho, rtol=1e-14, atol=0) and np.allclose(I_[0], I, rtol=1e-14, atol=0)
        assert T_.shape == (1, 3) and T_[0, 0] == 0.0 and np.allclose(T_[0], T, rtol=1e-14, atol=0)
        A, n_band = AN.site_windows([rec], slon, slat, 500.0, DT, sub, [1, 2, 5])
        want = [max(T[1] - T[0], T[2] - T[1]), T[2], T[2]]
        assert n_band == 0 and np.allclose(A[:, 0, 0], want, rtol=1e-14, atol=0)
        # the same total as the rainfall's trapezoid
        tot, _ = RN.site_values([rec], slon, slat, 500.0)
        assert math.isclose(A[2, 0, 0], tot[0, 0], rel_tol=1e-14)
    # r_out cuts records out: their rate is an exact 0, the others' terms stay
    rec = RN.records(lon, lat, v, DT, 2)[0]
    r = RN.haversine_km(rec[0], rec[1], slon[0], slat[0])
    cut = float(np.sort(r)[2] + np.sort(r)[3]) / 2
    inside, rho_, I_, T_, _ = AN.series(rec, slon, slat, cut, DT, 2)
    assert inside.sum() == 3 and (rho_[0][~inside[0]] == 0.0).all() and (rho_[0][inside[0]] > 0).all()
    # a NaN at sample k cuts the track: T has k boundaries
    lon8 = 280.0 + 0.2 * np.arange(8.0)[None, :]
    lat8, v8 = np.full((1, 8), 20.0), np.full((1, 8), 30.0)
    for k in range(8):
        vk = v8.copy()
        vk[0, k] = np.nan
        rec = RN.records(lon8, lat8, vk, DT, 3)[0]
        A, _ = AN.site_windows([rec], [280.3], [20.1], 500.0, DT, 3, [1, 4, 96])
        if k < 2:
            assert rec is None and np.isnan(A).all()
        else:
            T_ = AN.series(rec, [280.3], [20.1], 500.0, DT, 3)[3]
            assert T_.shape == (1, k) and A[2, 0, 0] == T_[0, -1] and A[0, 0, 0] <= A[1, 0, 0] <= A[2, 0, 0]
            if k - 1 <= 4:
                assert A[1, 0, 0] == A[2, 0, 0]
    # a 2-sample track: one interval, every window is the total
    lon2, lat2, v2 = np.array([[280.0, 280.2]]), np.array([[20.0, 20.0]]), np.array([[40.0, 40.0]])
    A, _ = AN.site_windows(RN.records(lon2, lat2, v2, DT, 1), [280.0], [20.0], 500.0, DT, 1, [1, 2, 5])
    r1 = float(RN.haversine_km(280.0, 20.0, 280.2, 20.0))
    assert np.allclose(A[:, 0, 0], 0.5 * (float(RN.rate(0.0, 40.0)) + float(RN.rate(r1, 40.0))), rtol=1e-14, atol=0)
    # a far site: NaN in every window
    far, _ = AN.site_windows(RN.records(lon2, lat2, v2, DT, 1), [100.0], [-20.0], 500.0, DT, 1, [1, 2, 5])
    assert np.isnan(far).all()
    # counts of the restatement's own values
    c = AN.counts(A, np.zeros(1, int), 2, [1.0, float(A[0, 0, 0]), 1e9])
    assert c.shape == (1, 2, 3, 3) and c[0, 0].tolist() == [[1, 1, 0]] * 3 and not c[:, 1].any()


def _stress(seed, r_out=400.0):
    from tests.test_rainfall import _groups, _stress_sites, _stress_tracks
    rng = np.random.default_rng(seed)
    lon, lat, v = _stress_tracks(rng)
    groups, n_groups = _groups(rng, lon.shape[0])
    slon, slat = _stress_sites(rng, lon, lat, v, r_out)
    return rng, lon, lat, v, groups, n_groups, slon, slat


@functools.lru_cache(maxsize=None)
def _stress_case(sub):
    """The stress input (140 storms x 48 samples, 70 sites) and the restatement on it, computed once and never changed."""
    _, lon, lat, v, groups, n_groups, slon, slat = _stress(61)
    recs = RN.records(lon, lat, v, DT, sub)
    A, n_band = AN.site_windows(recs, slon, slat, 400.0, DT, sub, STRESS_WINDOWS)
    total, _ = RN.site_values(recs, slon, slat, 400.0)
    peak, _ = RN.site_values(recs, slon, slat, 400.0, 'peak-rate')
    for a in (A, total, peak):
        a.setflags(write=False)
    return dict(tracks=(lon, lat, v, groups), n_groups=n_groups, sites=(slon, slat), recs=recs, A=A, n_band=n_band, total=total, peak=peak)


@pytest.mark.parametrize('sub', [1, 3])
def test_restatement_total_monotone_and_peak_bound(sub):
    d = _stress_case(sub)
    A, total, peak = d['A'], d['total'], d['peak']
    nan = np.isnan(total)
    assert (~nan).sum() > 300 and (np.isnan(A) == nan).all()
    # m >= n - 1: the storm total by the same trapezoid rule, up to the rounding of the two summations
    assert RN.close(A[4], total).all() and RN.close(A[5], total).all() and np.array_equal(A[4][~nan], A[5][~nan])
    # non-decreasing over the windows, exactly
    assert (np.diff(np.where(np.isnan(A), 0.0, A), axis=0) >= 0).all()
    assert (A[0][~nan] < A[3][~nan]).sum() > 200                       # and the windows do differ
    # A <= m dt_h peak
    for i, m in enumerate(STRESS_WINDOWS):
        assert (A[i][~nan] <= m * (DT / 3600.0) * peak[~nan] * (1 + 1e-12)).all()


def test_closed_form_window_of_a_straight_track():
    """A storm moving at c along a line through the site: the depth of a window of D hours is the integral of the rate over c D
    of path, and the largest one is where rate(start) = rate(end).  For D = 12 h (c D / 2 = 120 km > rm) that is the window
    centred on the passage, (2 / c) int_0^{c D / 2} rate(x) dx.  For D = 2 h (c D / 2 = 20 km < rm) the centred window is a
    stationary point too, but a minimum: with T0 < Tm the rate rises from the centre to rm, so the largest 2-hour depth lies
    astride rm (asserted below), and the reference is that window's integral."""
    from tests.test_rainfall import _equator_track
    c, n_t, vmax, r_out = 20.0, 48, 40.0, 300.0
    lon, lat, v = _equator_track(c, n_t, vmax)
    x_site = 23.37 * c                                                  # km along the track: between two samples
    slon = np.array([200.0 + np.rad2deg(x_site / RN.EARTH_R_KM)])
    t0, tm, rm, re = (float(x) * RN.MMH if i < 2 else float(x) for i, x in enumerate(RN.profile_terms(vmax)))
    assert 0 < t0 < tm and rm < r_out

    def rate(x):
        x = abs(x)
        return t0 + (tm - t0) * x / rm if x < rm else tm * math.exp(-(x - rm) / re)

    def F(x):                                                           # int_0^x rate, x >= 0
        return t0 * x + (tm - t0) * x * x / (2 * rm) if x <= rm else (t0 + tm) / 2 * rm + tm * re * (1.0 - math.exp(-(x - rm) / re))

    def G(x):
        return math.copysign(F(abs(x)), x)

    def exact(D):
        """(the largest depth of a window of D hours, its start in km relative to the site)"""
        W = c * D
        lo, hi = -W / 2, rm                                             # rate(a + W) - rate(a): 0 at -W / 2, < 0 at rm
        if rate(lo + 1e-3 + W) - rate(lo + 1e-3) <= 0:
            return (G(W / 2) - G(-W / 2)) / c, -W / 2                   # the centred window is the maximum
        lo += 1e-3
        for _ in range(200):
            mid = (lo + hi) / 2
            lo, hi = (mid, hi) if rate(mid + W) - rate(mid) > 0 else (lo, mid)
        return (G(lo + W) - G(lo)) / c, lo
    L = c * max(abs(tm - t0) / rm, tm / re)                             # Lipschitz constant of the rate in time (mm/h per h)
    for D in (2, 12):
        ex, a = exact(D)
        centred = (2.0 / c) * F(c * D / 2)
        if D == 12:
            assert a == -c * D / 2 and math.isclose(ex, centred, rel_tol=1e-14) and c * D / 2 > rm
        else:
            assert c * D / 2 < rm and 0 < a < rm < a + c * D and ex > centred
        # every window of c D km holds at most ex: a fine scan of the start
        assert max((G(s + c * D) - G(s)) / c for s in np.arange(-200.0, 200.0, 0.05)) <= ex * (1 + 1e-12)
        err = {}
        for sub in (1, 4, 16):
            h = DT / 3600.0 / sub
            A, n_band = AN.site_windows(RN.records(lon, lat, v, DT, sub), slon, np.array([0.0]), r_out, DT, sub, [D])
            assert n_band == 0
            err[sub] = abs(float(A[0, 0, 0]) - ex)
            # the trapezoid rule over D hours (the existing closed-form test's bound with T = D), and a window that starts up to
            # one sample interval away from the best start: at most that interval of the peak rate
            assert err[sub] <= L * h * D / 4 + 2 * h * tm + (DT / 3600.0) * tm, (D, sub, err[sub], ex)
        print('D = %d h: exact %.6f mm, |restatement - exact| at substeps 1, 4, 16: %.3g %.3g %.3g' % (D, ex, err[1], err[4], err[16]))
        assert err[16] < err[1]
    assert 10.0 < exact(2)[0] < 30.0 and 50.0 < exact(12)[0] < 150.0


def test_argument_errors_before_any_device_work(monkeypatch):
    from tropical_cyclone_risk_amd import _lib, accumulation, rainfall

    def no_library():
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', no_library)
    rng = np.random.default_rng(0)
    lon, lat, v = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    base = dict(lon=lon, lat=lat, vmax=v, groups=np.zeros(3, np.int64), site_lon=np.array([280.0]), site_lat=np.array([20.0]), dt_s=DT)
    a0, b0 = rainfall.DEFAULT_COEFFICIENTS
    bad = [dict(windows_h=[6.5]), dict(windows_h=[6, 12], dt_s=7 * 3600.0), dict(windows_h=[1], dt_s=3 * 3600.0),     # no multiple of dt_s
           dict(windows_h=[0]), dict(windows_h=[0, 6]), dict(windows_h=[-6]),                                         # 0 samples, fewer
           dict(windows_h=[97]), dict(windows_h=[6, 200]), dict(windows_h=[12], dt_s=400.0),                          # above 96 samples
           dict(windows_h=[12, 6]), dict(windows_h=[6, 6]),                                                           # not ascending
           dict(windows_h=np.arange(1, 10)), dict(windows_h=[]), dict(windows_h=[np.nan]),                            # 9 windows, none
           dict(windows_h=[1, 2, 3, 4, 5], thresholds=np.arange(1.0, 13.0)),                                          # 5 * 13 = 65 cells
           dict(windows_h=[1, 2, 3, 4, 5, 6, 7, 96], thresholds=np.arange(1.0, 8.0)),                                # 64 cells, 66048 bytes of LDS
           dict(return_values=[5]), dict(return_values=[0, 0]), dict(return_values='x'), dict(return_values=[0.5]),
           # the rainfall's own rules
           dict(substeps=0), dict(substeps=65), dict(substeps=1.5), dict(r_out_km=0.0), dict(r_out_km=2000.5), dict(dt_s=0.0),
           dict(dt_s=np.inf), dict(thresholds=np.array([20.0, 10.0])), dict(thresholds=np.array([])), dict(thresholds=np.array([10.0, np.inf])),
           dict(coefficients=(a0, (3.96, 4.80, -14.0, -16.0))), dict(coefficients=(a0, b0[:3])), dict(v_hi_kt=170.0), dict(v_lo_kt=0.0),
           dict(vmax=v[:, :4]), dict(groups=np.zeros(2, np.int64)), dict(site_lat=np.array([np.nan])), dict(site_lon=np.array([1.0, 2.0])),
           dict(groups=np.array([0, 1, 2]), n_groups=2), dict(n_groups=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            accumulation.site_accumulation(**dict(base, **kw))
    # the limits themselves pass the checks: 8 windows x 7 bins with 95 samples (65536 bytes), 96 samples alone
    accumulation._check_windows([1, 2, 3, 4, 5, 6, 7, 95], DT, np.arange(1.0, 8.0), True)
    _, m, want = accumulation._check_windows([48], 1800.0, [10.0], [0])
    assert m.tolist() == [96] and m.dtype == np.int32 and want == [0]
    _, m, want = accumulation._check_windows([6, 12, 24], 3 * 3600.0, THR, [2, 0])
    assert m.tolist() == [2, 4, 8] and want == [0, 2]
    # good arguments do reach the library
    with pytest.raises(AssertionError, match='the library was touched'):
        accumulation.site_accumulation(**base)
    with pytest.raises(AssertionError, match='the library was touched'):
        accumulation.site_accumulation(**dict(base, windows_h=[3, 96], substeps=4, return_values=[1]))


def test_defaults_and_cli_arguments(capsys):
    from tropical_cyclone_risk_amd import accumulation, analysis, rainfall
    assert accumulation.DEFAULT_WINDOWS_H == (6, 12, 24, 48, 72)
    a = accumulation.parse_args(['x.nc', '--site', '1,2'])
    assert a.windows.tolist() == [6, 12, 24, 48, 72] and np.array_equal(a.thresholds, rainfall.DEFAULT_RAIN_THRESHOLDS)
    assert a.r_out_km == 500.0 and a.substeps == 1 and a.out == 'accumulation.npz' and a.return_periods is None
    b = accumulation.parse_args(['x.nc', 'y.nc', '--grid', '270:271:0.5,20:21:1', '--windows', '6,24,72', '--thresholds', '20:60:10',
                                 '--substeps', '4', '--r-out-km', '300', '--return-periods', '10,50,100', '--out', 'ddf.npz'])
    assert b.tracks == ['x.nc', 'y.nc'] and b.windows.tolist() == [6, 24, 72] and b.thresholds.tolist() == [20, 30, 40, 50, 60]
    assert b.substeps == 4 and b.r_out_km == 300.0 and list(b.return_periods) == [10.0, 50.0, 100.0] and b.out == 'ddf.npz'
    assert analysis.collect_sites(b)[0].size == 6
    for argv in (['x.nc'], ['x.nc', '--site', '1,2', '--windows', '24,6'], ['x.nc', '--site', '1,2', '--windows', 'a,b'],
                 ['x.nc', '--site', '1,2', '--windows', '0,6'], ['x.nc', '--site', '1,2', '--windows', '1,2,3,4,5,6,7,8,9'],
                 ['x.nc', '--site', '1,2', '--return-periods', '10', '--tail-exceedances', '5']):
        with pytest.raises(SystemExit):
            accumulation.parse_args(argv)
    assert 'not offered' in capsys.readouterr().err


def test_accumulation_symbols_exported_and_abi_version_unchanged(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_accumulation_dev', 'tcr_accumulation_host', 'tcr_accumulation_pairs'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    L.tcr_abi_version.restype = ctypes.c_int
    assert L.tcr_abi_version() == 7 and _lib.TCR_ABI_VERSION == 7


# ------------------------------------------------------------------------------------------------------------------ GPU
def _compare(got, want, what):
    """NaN exactly where the restatement has NaN, values within the restatement's tolerance; prints the measured maxima."""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    d = np.abs(got - want)
    print('%s: %d values, largest |got - want| = %.3g, largest relative = %.3g'
          % (what, (~np.isnan(want)).sum(), np.nanmax(d), np.nanmax(d / np.maximum(np.abs(want), 1e-300))))
    bad = np.argwhere(~RN.close(got, want))
    assert len(bad) == 0, [(tuple(int(x) for x in i), got[tuple(i)], want[tuple(i)]) for i in bad[:5]]


@functools.lru_cache(maxsize=None)
def _stress_gpu(sub):
    from tropical_cyclone_risk_amd import accumulation
    d = _stress_case(sub)
    lon, lat, v, groups = d['tracks']
    return accumulation.site_accumulation(lon, lat, v, groups, d['sites'][0], d['sites'][1], DT, windows_h=STRESS_WINDOWS, thresholds=THR,
                                          r_out_km=400.0, substeps=sub, return_values=True, n_groups=d['n_groups'])


@pytest.mark.gpu
@pytest.mark.parametrize('sub', [1, 3])
def test_gpu_stress_matches_restatement(built_lib, sub):
    """Against TOL_ABS + TOL_REL |value| (accumulation_numpy's argument); measured on an MI355X: largest |got - want| 6.5e-13 mm,
    largest relative 2.2e-14, so the fallback of a bound relative to the storm total is not needed."""
    d = _stress_case(sub)
    A = d['A']
    assert [None if r is None else r.shape[1] for r in d['recs'][:6]] == [None, None, 1 + sub, 32 * sub + 1, 33 * sub + 1, 11 * sub + 1]
    assert d['n_band'] == 0 and not AN.near_threshold(A, THR).any()                 # decided on the CPU side
    r = _stress_gpu(sub)
    assert r['window_samples'].tolist() == STRESS_WINDOWS and r['windows_h'].tolist() == STRESS_WINDOWS
    got = r['site_window']
    _compare(got, A, 'substeps %d' % sub)
    assert r['counts'].dtype == np.int32 and np.array_equal(r['counts'], AN.counts(A, d['tracks'][3], d['n_groups'], THR))
    assert np.isnan(A[:, :, :2]).all() and np.isnan(A[:, :, 7]).all() and A[0, 0, 2] > 0
    assert (r['counts'][:, 1] == 0).all() and (r['counts'][:, 4] == 0).all() and r['counts'].sum() > 1000
    assert (np.diff(r['counts'], axis=2) >= 0).all() and (np.diff(r['counts'], axis=3) <= 0).all()


def _there_and_back():
    """20 km/h east along the equator for 200 km and back: 21 samples."""
    return np.concatenate([np.arange(0.0, 201.0, 20.0), np.arange(180.0, -1.0, -20.0)])


# name -> (sample positions in km of each storm, sites (km, lat), vmax, r_out, substeps, window lists, included records of
# (site, storm) pairs)
CATCH_UP = {
    # passes the site, leaves r_out and returns: records 2..7 and 13..18 at the first site; the second site has the track's
    # first record and its last.  [2, 4, 8, 16]: the gap of 5 boundaries is walked and one window spans both passes; [2] and
    # [1, 3]: the gap is longer than the ring (m_max + 1 = 3 and 4) and is jumped
    'return': ([_there_and_back()], [(90.0, 0.1), (10.0, 0.1)], 40.0, 60.0, 1, ([2, 4, 8, 16], [2], [1, 3]),
               {(0, 0): list(range(2, 8)) + list(range(13, 19)), (1, 0): [0, 1, 2, 3, 17, 18, 19, 20]}),
    'return, substeps 2': ([_there_and_back()], [(90.0, 0.1), (10.0, 0.1)], 40.0, 60.0, 2, ([2, 4, 8, 16], [2], [1, 3]),
                           {(0, 0): list(range(4, 15)) + list(range(26, 37)), (1, 0): list(range(0, 7)) + list(range(34, 41))}),
    # 40 km/h, substeps 4, r_out 15 km: the site's only records lie strictly between samples 3 and 4
    'between samples': ([40.0 * np.arange(8)], [(140.0, 0.05)], 40.0, 15.0, 4, ([1, 2, 5], [1]), {(0, 0): [13, 14, 15]}),
    # 33 samples at substeps 3 are 97 = 3 x 32 + 1 records, the last segment holds one; 34 samples are 100 records
    'last segment': ([20.0 * np.arange(33), 20.0 * np.arange(34)], [(630.0, 0.1), (650.0, 0.1)], 55.0, 60.0, 3, ([2, 4, 8, 16], [1]),
                     {(0, 0): list(range(86, 97)), (1, 1): list(range(89, 100)), (1, 0): list(range(89, 97))}),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CATCH_UP))
def test_gpu_catch_up_paths(built_lib, name):
    from tropical_cyclone_risk_amd import accumulation
    xs, sites, vmax, r_out, sub, window_lists, included = CATCH_UP[name]
    n_t = max(len(x) for x in xs)
    lon, lat, v = (np.concatenate(p) for p in zip(*[_km_track(x, vmax, n_t) for x in xs]))
    slon, slat = (np.concatenate(p) for p in zip(*[_site_km(*s) for s in sites]))
    recs = RN.records(lon, lat, v, DT, sub)
    for (i, s), want in included.items():                               # the structure the case is about
        inside = AN.series(recs[s], slon[i:i + 1], slat[i:i + 1], r_out, DT, sub)[0]
        assert np.flatnonzero(inside[0]).tolist() == want, (name, i, s, np.flatnonzero(inside[0]).tolist())
        assert recs[s].shape[1] == (len(xs[s]) - 1) * sub + 1
    for windows in window_lists:
        A, n_band = AN.site_windows(recs, slon, slat, r_out, DT, sub, windows)
        assert n_band == 0
        r = accumulation.site_accumulation(lon, lat, v, np.zeros(len(xs), np.int64), slon, slat, DT, windows_h=windows, thresholds=[1.0, 10.0],
                                           r_out_km=r_out, substeps=sub, return_values=True)
        _compare(r['site_window'], A, '%s, windows %s' % (name, windows))
        assert not AN.near_threshold(A, [1.0, 10.0]).any() and np.array_equal(r['counts'], AN.counts(A, np.zeros(len(xs), int), 1, [1.0, 10.0]))
    if name == 'return':                                                # one window does span both passes
        A, _ = AN.site_windows(recs, slon, slat, r_out, DT, sub, [4, 16])
        assert A[1, 0, 0] > 1.5 * A[0, 0, 0]


@pytest.mark.gpu
def test_gpu_consistent_with_the_rainfall_footprint(built_lib):
    from tropical_cyclone_risk_amd import rainfall
    for sub in (1, 3):
        d, r = _stress_case(sub), _stress_gpu(sub)
        lon, lat, v, groups = d['tracks']
        kw = dict(r_out_km=400.0, substeps=sub, n_groups=d['n_groups'], return_values=True)
        total = rainfall.site_rain(lon, lat, v, groups, d['sites'][0], d['sites'][1], DT, thresholds=THR, **kw)['site_total']
        peak = rainfall.site_rain(lon, lat, v, groups, d['sites'][0], d['sites'][1], DT, stat='peak-rate', thresholds=THR, **kw)['site_peak_rate']
        sw = r['site_window']
        nan = np.isnan(total)
        assert (np.isnan(sw) == nan).all() and np.array_equal(np.isnan(peak), nan) and (~nan).sum() > 300
        print('substeps %d: largest |longest window - site_total| = %.3g' % (sub, np.nanmax(np.abs(sw[-1] - total))))
        assert RN.close(sw[-1], total).all() and RN.close(sw[-2], total).all()
        assert (np.diff(np.where(np.isnan(sw), 0.0, sw), axis=0) >= 0).all()          # as numbers, exactly
        for i, m in enumerate(STRESS_WINDOWS):
            assert (sw[i][~nan] <= m * (DT / 3600.0) * peak[~nan] * (1 + 1e-12)).all()


@pytest.mark.gpu
def test_gpu_bit_identical_across_runs_site_order_storm_order_and_site_count(built_lib):
    """The guard of the order guarantee: the windows of a (site, storm) are the same bits whichever lane, tile and chunk computed
    them and whatever was culled around them (substeps 3: runs of included records cross culled segments)."""
    import torch
    from tropical_cyclone_risk_amd import accumulation
    rng, lon, lat, v, groups, n_groups, slon, slat = _stress(5, 500.0)
    n_trk = lon.shape[0]
    dev = torch.device('cuda', 0)
    tl, ta, tv, sl, sa = (torch.as_tensor(x, device=dev) for x in (lon, lat, v, slon, slat))
    kw = dict(windows_h=[1, 3, 6, 24, 47], thresholds=THR, r_out_km=500.0, substeps=3, return_values=True, n_groups=n_groups)

    def same(x, y):
        return torch.equal(x.view(torch.int64), y.view(torch.int64))               # bits: NaN equal to NaN
    a = accumulation.site_accumulation(tl, ta, tv, groups, sl, sa, DT, **kw)
    assert (~torch.isnan(a['site_window'][0])).sum() > 500
    b = accumulation.site_accumulation(tl, ta, tv, groups, sl, sa, DT, **kw)
    assert same(a['site_window'], b['site_window']) and torch.equal(a['counts'], b['counts'])
    ps = torch.as_tensor(rng.permutation(slon.size), device=dev)
    c = accumulation.site_accumulation(tl, ta, tv, groups, sl[ps], sa[ps], DT, **kw)
    assert same(c['site_window'], a['site_window'][:, ps]) and torch.equal(c['counts'], a['counts'][ps])
    pt = np.arange(n_trk)                                                   # storms permuted within their groups
    for g in range(n_groups):
        i = np.nonzero(groups == g)[0]
        pt[i] = rng.permutation(i)
    assert np.array_equal(groups[pt], groups) and not np.array_equal(pt, np.arange(n_trk))
    tp = torch.as_tensor(pt, device=dev)
    d = accumulation.site_accumulation(tl[tp], ta[tp], tv[tp], groups, sl, sa, DT, **kw)
    assert same(d['site_window'], a['site_window'][:, :, tp]) and torch.equal(d['counts'], a['counts'])
    px = rng.permutation(n_trk)                                             # ... and across groups, the groups going along
    tx = torch.as_tensor(px, device=dev)
    e = accumulation.site_accumulation(tl[tx], ta[tx], tv[tx], groups[px], sl, sa, DT, **kw)
    assert same(e['site_window'], a['site_window'][:, :, tx]) and torch.equal(e['counts'], a['counts'])
    # 200 far sites more: other tiles, another grid, the same 70 rows
    fl_ = torch.as_tensor(rng.uniform(0.0, 40.0, 200), device=dev)
    fa_ = torch.as_tensor(rng.uniform(55.0, 80.0, 200), device=dev)
    f = accumulation.site_accumulation(tl, ta, tv, groups, torch.cat([sl, fl_]), torch.cat([sa, fa_]), DT, **kw)
    assert same(f['site_window'][:, :70], a['site_window']) and torch.equal(f['counts'][:70], a['counts'])
    assert torch.isnan(f['site_window'][:, 70:]).all() and int(f['counts'][70:].sum()) == 0
    # a window alone gives the bits it has in the joint call
    g1 = accumulation.site_accumulation(tl, ta, tv, groups, sl, sa, DT, **dict(kw, windows_h=[6]))
    assert same(g1['site_window'][0], a['site_window'][2]) and torch.equal(g1['counts'][:, :, 0], a['counts'][:, :, 2])


@pytest.mark.gpu
def test_gpu_host_and_device_entry_points_agree_and_pairs(built_lib):
    import torch
    from tropical_cyclone_risk_amd import _lib, accumulation, rainfall
    from tropical_cyclone_risk_amd.engine import TCEngine
    d, ref = _stress_case(3), _stress_gpu(3)
    lon, lat, v, groups = d['tracks']
    slon, slat = d['sites']
    n_groups = d['n_groups']
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(x, device=dev) for x in (lon, lat, v, slon, slat)]
    eng = TCEngine('NA', device=0)
    L = _lib.lib()
    pairs, rpairs = ctypes.c_int64(-1), ctypes.c_int64(-1)
    side = torch.cuda.Stream(dev)
    kw = dict(windows_h=STRESS_WINDOWS, thresholds=THR, r_out_km=400.0, substeps=3, n_groups=n_groups, engine=eng)
    try:
        # no accumulation call on this context yet: an error with a message, not a number
        assert L.tcr_accumulation_pairs(eng.h, ctypes.byref(pairs)) == -1
        assert L.tcr_last_error(eng.h).decode().startswith('tcr_accumulation_pairs: no tcr_accumulation_* call')
        h = accumulation.site_accumulation(lon, lat, v, groups, slon, slat, DT, return_values=True, **kw)              # _host
        assert LN.same_bits(h['site_window'], ref['site_window']) and np.array_equal(h['counts'], ref['counts'])
        assert L.tcr_accumulation_pairs(eng.h, ctypes.byref(pairs)) == 0
        rainfall.site_rain(lon, lat, v, groups, slon, slat, DT, r_out_km=400.0, substeps=3, thresholds=THR, n_groups=n_groups, engine=eng)
        assert L.tcr_rainfall_pairs(eng.h, ctypes.byref(rpairs)) == 0 and 0 < pairs.value == rpairs.value   # the footprint's pairs
        for want in (True, [4, 1], False):
            for stream in (side, torch.cuda.current_stream(dev)):
                with torch.cuda.stream(stream):
                    r = accumulation.site_accumulation(t[0], t[1], t[2], groups, t[3], t[4], DT, return_values=want, **kw)  # _dev
                stream.synchronize()
                assert r['counts'].device == dev and np.array_equal(r['counts'].cpu().numpy(), ref['counts'])
                if want is False:
                    assert 'site_window' not in r
                    continue
                got = r['site_window'].cpu().numpy()
                assert r['site_window'].device == dev
                for i in range(len(STRESS_WINDOWS)):                    # planes for a subset: the others are NaN, nothing else moves
                    assert LN.same_bits(got[i], ref['site_window'][i]) if want is True or i in want else np.isnan(got[i]).all()
        # no storms at all
        z = accumulation.site_accumulation(lon[:0], lat[:0], v[:0], groups[:0], slon, slat, DT, return_values=True, **dict(kw, n_groups=2))
        assert z['counts'].shape == (70, 2, 6, 9) and z['counts'].sum() == 0 and z['site_window'].shape == (6, 70, 0)
        zt = accumulation.site_accumulation(t[0][:0], t[1][:0], t[2][:0], groups[:0], t[3], t[4], DT, **dict(kw, n_groups=2))
        assert int(zt['counts'].sum()) == 0
        assert L.tcr_accumulation_pairs(eng.h, ctypes.byref(pairs)) == 0 and pairs.value == 0
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_abi_rejects_bad_arguments(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        n_trk, n_t = 2, 6
        planes = [np.full((n_trk, n_t), x) for x in (280.0, 20.0, 30.0)]
        planes[0] = planes[0] + 0.1 * np.arange(n_t)
        off = (ctypes.c_int64 * 2)(0, n_trk)
        s = np.array([280.2]), np.array([20.0])
        a0, b0 = (-1.10, -1.60, 64.5, 150.0), (3.96, 4.80, -13.0, -16.0)

        def call(windows=(1, 3), thr=(10.0, 20.0), planes_out=True, **p):
            trk = _lib.HazardTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=planes[0].ctypes.data, lat=planes[1].ctypes.data,
                                    vmax=planes[2].ctypes.data, n_group=1, group_off=off)
            prm = _lib.RainParams(**dict(dict(dt_s=DT, r_out_km=500.0, v_lo_kt=35.0, v_hi_kt=155.0, a=(ctypes.c_double * 4)(*a0),
                                              b=(ctypes.c_double * 4)(*b0), substeps=1, stat=0), **p))
            m, th = np.asarray(windows, np.int32), np.asarray(thr, float)
            n_w = len(windows)
            counts = np.full((1, 1, max(n_w, 1), len(thr)), -7, np.int32)
            sw = np.full((max(n_w, 1), 1, n_trk), -7.0)
            arr = (ctypes.c_void_p * max(n_w, 1))()
            for i in range(min(n_w, 8)):
                arr[i] = sw[i].ctypes.data
            rc = L.tcr_accumulation_host(h, ctypes.byref(trk), ctypes.byref(prm), 1, s[0].ctypes.data, s[1].ctypes.data, n_w,
                                         m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(thr), th.ctypes.data_as(_lib.DP),
                                         counts.ctypes.data, arr if planes_out else None)
            return rc, counts, sw
        pairs = ctypes.c_int64()
        rejected = [dict(stat=1), dict(windows=()), dict(windows=tuple(range(1, 10))), dict(windows=(0, 3)), dict(windows=(3, 97)),
                    dict(windows=(3, 3)), dict(windows=(6, 3)),
                    dict(windows=(1, 2, 3, 4, 5), thr=np.arange(1.0, 13.0)),                           # 65 cells
                    dict(windows=(1, 2, 3, 4, 5, 6, 7, 96), thr=np.arange(1.0, 8.0)),                  # 64 cells, 66048 bytes of LDS
                    dict(r_out_km=2001.0), dict(substeps=0), dict(substeps=65), dict(dt_s=0.0), dict(stat=2), dict(v_lo_kt=0.0),
                    dict(thr=(20.0, 10.0)), dict(thr=())]
        for p in rejected:
            assert call(**p)[0] == -1, p
            assert L.tcr_last_error(h).decode().startswith('tcr_accumulation:'), (p, L.tcr_last_error(h))
        # none of them got as far as a launch: the context has still seen no accumulation call
        assert L.tcr_accumulation_pairs(h, ctypes.byref(pairs)) == -1
        rc, counts, sw = call()
        assert rc == 0 and counts.sum() > 0 and (counts >= 0).all() and (sw > 0).all() and (sw[0] < sw[1]).all()
        assert L.tcr_accumulation_pairs(h, ctypes.byref(pairs)) == 0 and pairs.value == n_trk * n_t
        rc, c2, s2 = call(planes_out=False)                                 # no planes: the counts are what they were
        assert rc == 0 and np.array_equal(c2, counts) and (s2 == -7).all()
        assert call(windows=(1, 2, 3, 4, 5, 6, 7, 95), thr=np.arange(1.0, 8.0))[0] == 0               # 65536 bytes
        assert call(windows=(96,), thr=(10.0,))[0] == 0
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_next_to_a_rainfall_call_on_two_streams_and_nothing_existing_moved(built_lib):
    """The context's seventh workspace: an accumulation call and a rainfall call in flight on two streams of one context give what
    they give one after the other; and the rainfall's total and peak rate are the same bits before and after an accumulation call."""
    import torch
    from tropical_cyclone_risk_amd import accumulation, rainfall
    from tropical_cyclone_risk_amd.engine import TCEngine
    _, lon, lat, v, groups, n_groups, slon, slat = _stress(12, 500.0)
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(x, device=dev) for x in (lon, lat, v, slon, slat)]
    eng = TCEngine('NA', device=0)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)

    def rain(stat='total'):
        return rainfall.site_rain(t[0], t[1], t[2], groups, t[3], t[4], DT, stat=stat, substeps=4, thresholds=THR, return_values=True,
                                  n_groups=n_groups, engine=eng)

    def accum():
        return accumulation.site_accumulation(t[0], t[1], t[2], groups, t[3], t[4], DT, windows_h=[3, 12, 47], substeps=4, thresholds=THR,
                                              return_values=True, n_groups=n_groups, engine=eng)

    def same(x, y):
        return torch.equal(x.view(torch.int64), y.view(torch.int64))
    try:
        r0, p0 = rain(), rain('peak-rate')
        a0 = accum()
        r2, p2 = rain(), rain('peak-rate')
        torch.cuda.synchronize(dev)
        assert same(r2['site_total'], r0['site_total']) and same(p2['site_peak_rate'], p0['site_peak_rate'])
        assert torch.equal(r2['counts'], r0['counts']) and torch.equal(p2['counts'], p0['counts'])
        for _ in range(3):
            with torch.cuda.stream(s1):
                a1 = accum()
            with torch.cuda.stream(s2):
                r1 = rain()
            s1.synchronize()
            s2.synchronize()
            assert same(a1['site_window'], a0['site_window']) and same(r1['site_total'], r0['site_total'])
            assert torch.equal(a1['counts'], a0['counts']) and torch.equal(r1['counts'], r0['counts'])
        assert int(r0['counts'].sum()) > 0 and int(a0['counts'].sum()) > 0
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_golden_tracks_on_a_site_grid(built_lib):
    from tests.test_rainfall import _golden
    from tropical_cyclone_risk_amd import accumulation
    lon, lat, vmax = _golden()
    groups = np.arange(lon.shape[0]) % 3
    glon, glat = np.meshgrid(np.arange(-100.3, 361.0, 8.0), np.arange(-48.3, 49.0, 8.0))
    slon, slat = glon.ravel(), glat.ravel()
    A, n_band = AN.site_windows(RN.records(lon, lat, vmax, DT, 1), slon, slat, 500.0, DT, 1, [6, 24, 72])
    assert n_band == 0 and not AN.near_threshold(A, THR).any()
    r = accumulation.site_accumulation(lon, lat, vmax, groups, slon, slat, DT, windows_h=[6, 24, 72], thresholds=THR, return_values=True)
    _compare(r['site_window'], A, 'golden tracks')
    assert np.array_equal(r['counts'], AN.counts(A, groups, 3, THR))
    assert (~np.isnan(A[0])).sum() > 500 and r['counts'].sum() > 200


@pytest.mark.gpu
def test_gpu_run_downscaling_tracks_then_cli(golden_env, built_lib, tmp_path, capsys):
    from tests.test_rainfall import _nl
    from tropical_cyclone_risk_amd import accumulation, analysis, compute, hazard, io as tio, levels
    nl = _nl(start_year=2001, end_year=2003, tracks_per_year=40, dataset_type='SYNTHETIC', output_directory=str(tmp_path), exp_name='ac')
    os.makedirs(tmp_path / 'ac', exist_ok=True)
    fn = compute.run_downscaling('NA', env=golden_env, nl=nl)
    d = tio.read_tracks(fn)
    lon, lat, vmax = (np.asarray(d[k], float) for k in ('lon_trks', 'lat_trks', 'vmax_trks'))
    dt = analysis.sample_spacing([d['time']])
    assert dt == 3600.0
    groups = np.asarray(d['tc_years']).astype(int) - 2001
    i = np.argwhere(np.isfinite(lon) & np.isfinite(vmax))[::53][:8]
    slon = np.concatenate([lon[i[:, 0], i[:, 1]] - 360.0, [100.0]])          # the last one: the southern Indian Ocean, far from every track
    slat = np.concatenate([lat[i[:, 0], i[:, 1]] + 0.7, [-45.0]])
    out = str(tmp_path / 'accumulation.npz')
    argv = [fn, '--out', out, '--substeps', '2', '--windows', '6,24,72', '--thresholds', '5:100:5', '--return-periods', '2,5']
    argv += ['--site=%.12f,%.12f' % (a, b) for a, b in zip(slon, slat)]
    assert accumulation.main(argv) == 0
    text = capsys.readouterr().out
    assert 'windows 6,24,72 h' in text and 'return period' in text
    z = np.load(out)
    assert set(z.files) == {'counts', 'return_period', 'windows_h', 'window_samples', 'thresholds', 'site_lon', 'site_lat', 'total_years',
                            'r_out_km', 'substeps', 'dt_s', 'group_file', 'group_year', 'files', 'return_level', 'return_periods', 'n_reach'}
    assert int(z['total_years']) == 3 and z['window_samples'].tolist() == [6, 24, 72] and z['windows_h'].tolist() == [6, 24, 72]
    thr = np.arange(5.0, 101.0, 5.0)
    api = accumulation.site_accumulation(lon, lat, vmax, groups, z['site_lon'], z['site_lat'], dt, windows_h=[6, 24, 72], thresholds=thr,
                                         substeps=2, n_groups=3, return_values=True)
    assert np.array_equal(z['counts'], api['counts']) and api['counts'].sum() > 0 and z['counts'].shape == (9, 3, 3, 20)
    assert np.array_equal(z['return_period'], hazard.return_periods(api['counts'], 3))
    k, ok = levels.ranks_of_periods([2.0, 5.0], 3)
    assert z['return_level'].shape == (9, 3, 2) and np.array_equal(z['return_periods'], [2.0, 5.0])
    for w in range(3):
        want, n_reach = LN.row_select(api['site_window'][w], k)
        want[:, ~ok] = np.nan
        assert LN.same_bits(z['return_level'][:, w], want) and np.array_equal(z['n_reach'], n_reach)
    assert not np.isnan(z['return_level'][:8, :, 0]).any() and np.isnan(z['return_level'][8]).all()
    assert (np.diff(z['return_level'][:8, :, 0], axis=1) >= 0).all()                # the DDF table rises with the duration
    # the API's values are the restatement's on this file too
    A, _ = AN.site_windows(RN.records(lon, lat, vmax, dt, 2), z['site_lon'], z['site_lat'], 500.0, dt, 2, [6, 24, 72])
    assert RN.close(api['site_window'], A).all()
