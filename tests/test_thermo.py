"""PI / chi / RH preprocessing: oracle vs the reference's golden vectors (CPU),
HIP kernels vs oracle and golden (GPU).

The second half pins the kernels branch by branch on the column family of tests/thermo_columns.py at ERA5's own 37
levels: the oracle is pinned to the reference on those inputs, a census makes the family's coverage a condition, and
the kernels are held to the oracle by one rule (`_check_pi`, `_check_chi_rh`).

    python -m pytest tests/test_thermo.py -q -s            # prints the census and every measured maximum
"""
import os

import numpy as np
import pytest

from tests import thermo_columns as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FAMILY_SEED, FAMILY_N = 20261020, 1500


@pytest.fixture(scope='module')
def cases():
    return np.load(os.path.join(GOLDEN, 'thermo_cases.npz'))


@pytest.fixture(scope='module')
def table():
    return np.load(os.path.join(GOLDEN, 'entropy_table.npz'))


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_oracle_matches_reference(cases, table, tag):
    from oracle import thermo_oracle as to
    tb = to.Table(table['p'], table['s'], table['T'])
    p, sst, psl, T, r = (cases[tag + '_' + k] for k in ('p', 'sst', 'psl', 'T', 'r'))
    k_mid = int(cases[tag + '_k_mid'])
    pi, chi, rh = to.column_fields(tb, float(cases['Ck_over_Cd']), p, sst, psl, T, r, k_mid)
    # same formulas, same libm: the scalar restatement reproduces the vectorised reference to rounding
    np.testing.assert_allclose(pi, cases[tag + '_PI'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(chi, cases[tag + '_chi'], rtol=1e-12, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(rh, cases[tag + '_rh_mid'], rtol=1e-13, atol=0, equal_nan=True)
    for idx in [(0, 0), (1, 1), (2, 2), (5, 5), (7, 3)]:
        aux = to.potential_intensity(tb, 1.0, float(sst[idx]), float(psl[idx]), p, T[(slice(None),) + idx], r[(slice(None),) + idx])[1]
        np.testing.assert_allclose(aux['p_lcl'], cases[tag + '_pLCL'][idx], rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose(aux['s_ns'], cases[tag + '_s_ns'][idx], rtol=1e-13, equal_nan=True)
        np.testing.assert_allclose(aux['ss'], cases[tag + '_ss'][idx], rtol=1e-13, equal_nan=True)


def _gpu_fields(eng, table, cases, tag):
    from tropical_cyclone_risk_amd import preprocess as pp
    pp.stage_entropy_table(eng, table['p'], table['s'], table['T'])
    p, sst, psl, T, r = (cases[tag + '_' + k] for k in ('p', 'sst', 'psl', 'T', 'r'))
    k_mid = int(cases[tag + '_k_mid'])
    pi = pp.potential_intensity(eng, sst, psl, p, T, r)
    chi, rh = pp.chi_rh(eng, sst, psl, T[k_mid], r[k_mid], float(p[k_mid]))
    return pi, chi, rh


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_kernels_match_reference_golden(cases, table, built_lib, tag):
    """k_potential_intensity / k_chi_rh against the reference's own outputs.  Tolerance: 1e-9 relative
    (device libm vs glibc in exp/log/pow, own Lambert W); zeros and NaN-handling cases must agree exactly."""
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0)
    pi, chi, rh = _gpu_fields(eng, table, cases, tag)
    eng.close()
    ref = cases[tag + '_PI']
    assert np.array_equal(pi == 0, ref == 0)
    err = np.abs(pi - ref) / np.maximum(ref, 1.0)
    print('PI: max rel err %.2e, p99 %.2e' % (err.max(), np.percentile(err, 99)))
    assert err.max() < 1e-9
    np.testing.assert_allclose(chi, cases[tag + '_chi'], rtol=1e-9, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(rh, cases[tag + '_rh_mid'], rtol=1e-12, atol=0, equal_nan=True)


@pytest.mark.gpu
def test_compute_thermo_host_mirror(cases, table, built_lib):
    """calc_thermo.compute_thermo's array handling: level order, hPa, mid-level pick, chi clip."""
    from tropical_cyclone_risk_amd import preprocess as pp
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0)
    pi, chi, rh = _gpu_fields(eng, table, cases, 'b')
    p, sst, psl, T, r = (cases['b_' + k] for k in ('p', 'sst', 'psl', 'T', 'r'))
    v2, c2, r2 = pp.compute_thermo(eng, sst, psl, (p / 100)[::-1], 'hPa', T[::-1], r[::-1])     # top-down, hPa
    # (p / 100) * 100 is not p bit for bit, so agreement is to rounding, not exact
    np.testing.assert_allclose(v2, pi, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r2, rh, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(c2, np.minimum(np.maximum(chi, 0), 10), rtol=1e-9, atol=1e-12, equal_nan=True)
    assert np.nanmin(c2) >= 0 and np.nanmax(c2) <= 10
    with pytest.raises(Exception, match='lowest'):
        dp = lambda a: np.ascontiguousarray(a).ctypes.data_as(pp._lib.DP)
        out = np.empty(sst.shape)
        eng._ck(eng.L.tcr_potential_intensity_host(eng.h, sst.size, len(p), dp(p[::-1].copy()), dp(sst), dp(psl), dp(T), dp(r), 1.0, dp(out)))
    eng2 = TCEngine('GL', device=0)
    with pytest.raises(Exception, match='entropy table'):
        pp.potential_intensity(eng2, sst, psl, p, T, r)
    eng.close(); eng2.close()


def _nc3(fn, dims, variables):
    """variables: name -> (dims tuple, array, attrs)"""
    from scipy.io import netcdf_file
    with netcdf_file(fn, 'w', version=2) as f:
        for k, n in dims.items():
            f.createDimension(k, n)
        for name, (d, arr, attrs) in variables.items():
            a = np.asarray(arr)
            v = f.createVariable(name, 'f' if a.dtype == np.float32 else 'd', d)
            v[:] = a
            for k, x in attrs.items():
                setattr(v, k, x)


@pytest.mark.gpu
def test_file_drivers_wind_and_thermo(cases, table, built_lib, tmp_path):
    """gen_wind_mean_cov / gen_thermo over NetCDF files in the ERA5 layout of namelist.var_keys: daily u, v
    on (time, level, latitude, longitude) -> env_wnd file; monthly sst / sp / t / q -> thermo file; both are
    then read back through the field loader's dataset facade."""
    import datetime, types
    from oracle import wind_stats as ws
    from tropical_cyclone_risk_amd import fields, namelist, preprocess as pp
    from tropical_cyclone_risk_amd.engine import TCEngine
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    nl.dataset_type = 'ERA5'; nl.start_year, nl.start_month, nl.end_year, nl.end_month = 2001, 1, 2001, 3
    eng = TCEngine('GL', device=0, nl=nl)
    rng = np.random.default_rng(5)
    # ---- daily winds, Jan 1 .. Mar 31 2001, three levels in hPa
    nt, lat, lon = 90, np.linspace(-30, 30, 13), np.arange(0, 60, 5.0)
    days = np.arange(nt, dtype=float)
    lev = np.array([850.0, 500.0, 250.0])
    u = rng.normal(size=(nt, 3, len(lat), len(lon))).astype(np.float32)
    v = rng.normal(size=(nt, 3, len(lat), len(lon))).astype(np.float32)
    common = {'time': (('time',), days, dict(units='days since 2001-01-01 00:00:00', calendar='standard')),
              'level': (('level',), lev, dict(units='hPa')), 'latitude': (('latitude',), lat, {}), 'longitude': (('longitude',), lon, {})}
    dims = dict(time=nt, level=3, latitude=len(lat), longitude=len(lon))
    for name, arr in (('u', u), ('v', v)):
        _nc3(str(tmp_path / ('era5_%s_daily.nc' % name)), dims, dict(common, **{name: (('time', 'level', 'latitude', 'longitude'), arr, {})}))
    out = pp.gen_wind_mean_cov(eng, [str(tmp_path / 'era5_u_daily.nc')], [str(tmp_path / 'era5_v_daily.nc')], str(tmp_path / 'env_wnd.nc'), nl)
    ds = fields._Dataset(out)
    t = [datetime.datetime(2001, 1, 1) + datetime.timedelta(days=float(x)) for x in ds['time']]
    assert [(x.month, x.day) for x in t] == [(1, 1), (2, 15), (3, 15)]          # env_wind.py:139-152 stamps
    for k, (m0, m1) in enumerate([(0, 31), (31, 59), (59, 90)]):
        ref = ws.wind_stats([u[m0:m1, 2], v[m0:m1, 2], u[m0:m1, 0], v[m0:m1, 0]])
        assert np.array_equal(ds['ua250_Mean'][k], ref[0]) and np.array_equal(ds['va850_Mean'][k], ref[3])
        assert np.array_equal(ds['ua250_Var'][k], ref[4]) and np.array_equal(ds['va250_ua250_cov'][k], ref[5])
        assert np.array_equal(ds['va850_Var'][k], ref[13]) and np.array_equal(ds['va850_ua850_cov'][k], ref[12])
    # ---- monthly thermo: the golden soundings of case b as two monthly records; sst in Celsius on its own grid
    p, sst, psl, T, r = (cases['b_' + k] for k in ('p', 'sst', 'psl', 'T', 'r'))
    nla, nlo = sst.shape
    lat, lon = np.linspace(-40, 40, nla), np.linspace(100, 100 + 2.0 * (nlo - 1), nlo)
    tm = np.array([14.0, 45.0])
    tv = ('time', (('time',), tm, dict(units='days since 2001-01-01', calendar='standard')))
    ax = dict([tv, ('latitude', (('latitude',), lat, {})), ('longitude', (('longitude',), lon, {}))])
    d2 = dict(time=2, latitude=nla, longitude=nlo)
    _nc3(str(tmp_path / 'sst.nc'), d2, dict(ax, sst=(('time', 'latitude', 'longitude'), np.stack([sst, sst]) - 273.15, dict(units='degC'))))
    _nc3(str(tmp_path / 'sp.nc'), d2, dict(ax, sp=(('time', 'latitude', 'longitude'), np.stack([psl, psl]), dict(units='Pa'))))
    d3 = dict(d2, level=len(p))
    axl = dict(ax, level=(('level',), p[::-1] / 100.0, dict(units='hPa')))              # top-down in hPa, as ERA5 delivers
    # temperature comes as two files of one record each (open_mfdataset over a sorted glob, util/input.py:14-58)
    d31 = dict(d3, time=1)
    for j, day in enumerate(tm):
        ax1 = dict(axl, time=(('time',), np.array([day]), dict(units='days since 2001-01-01', calendar='standard')))
        _nc3(str(tmp_path / ('t_%d.nc' % j)), d31, dict(ax1, t=(('time', 'level', 'latitude', 'longitude'), T[::-1][None], {})))
    _nc3(str(tmp_path / 'q.nc'), d3, dict(axl, q=(('time', 'level', 'latitude', 'longitude'), np.stack([r[::-1], r[::-1]]), {})))
    out = pp.gen_thermo(eng, str(tmp_path / 'sst.nc'), [str(tmp_path / 'sp.nc')], [str(tmp_path / 't_0.nc'), str(tmp_path / 't_1.nc')], str(tmp_path / 'q.nc'),
                        str(tmp_path / 'thermo.nc'), nl, table=(table['p'], table['s'], table['T']))
    ds = fields._Dataset(out)
    assert ds['vmax'].shape == (2, nla, nlo)
    tt = [datetime.datetime(2001, 1, 1) + datetime.timedelta(days=float(x)) for x in ds['time']]
    assert [(x.month, x.day) for x in tt] == [(1, 15), (2, 15)]
    ok = cases['b_PI'] > 0
    # sst went through Celsius and back and the levels through hPa: agreement to rounding
    np.testing.assert_allclose(ds['vmax'][0][ok], cases['b_PI'][ok], rtol=1e-7)
    np.testing.assert_allclose(ds['vmax'][1], ds['vmax'][0], rtol=0, atol=0)
    assert np.nanmin(ds['chi']) >= 0 and np.nanmax(ds['chi']) <= 10
    eng.close()


@pytest.mark.gpu
def test_device_pointer_entry_points(cases, table, built_lib):
    """tcr_potential_intensity_dev / tcr_wind_stats_dev (device buffers, caller's stream) give what the host
    entry points give."""
    import ctypes as C
    import torch
    from tropical_cyclone_risk_amd import preprocess as pp
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0)
    pp.stage_entropy_table(eng, table['p'], table['s'], table['T'])
    p, sst, psl, T, r = (cases['a_' + k] for k in ('p', 'sst', 'psl', 'T', 'r'))
    ref = pp.potential_intensity(eng, sst, psl, p, T, r)
    dev = torch.device('cuda', 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    dp, dsst, dpsl, dT, dr = t(p), t(sst.ravel()), t(psl.ravel()), t(T.reshape(len(p), -1)), t(r.reshape(len(p), -1))
    out = torch.empty(sst.size, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    eng._ck(eng.L.tcr_potential_intensity_dev(eng.h, sst.size, len(p), dp.data_ptr(), dsst.data_ptr(), dpsl.data_ptr(),
                                              dT.data_ptr(), dr.data_ptr(), float(cases['Ck_over_Cd']), out.data_ptr(), C.c_void_p(st)))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(sst.shape), ref)
    rng = np.random.default_rng(2)
    planes = [rng.normal(size=(20, 500)) for _ in range(4)]
    want = eng.wind_stats(planes)
    dpl = [t(x) for x in planes]
    ptrs = (C.c_void_p * 4)(*[x.data_ptr() for x in dpl])
    o2 = torch.empty(14, 500, dtype=torch.float64, device=dev)
    eng._ck(eng.L.tcr_wind_stats_dev(eng.h, 20, 500, ptrs, None, 0, o2.data_ptr(), C.c_void_p(st)))
    torch.cuda.synchronize()
    assert np.array_equal(o2.cpu().numpy(), want)
    eng.close()


# --------------------------------------------------------------------------------------
# every branch of the fold, at ERA5's own levels
#
# The comparison rule.  k_potential_intensity and the oracle take a square root of x = Ck/Cd * sst / T_out * (CAPE* - CAPE),
# a difference of two sums, so an error in PI is unbounded relative to PI where x is small.  The kernel is therefore held
# to x itself, relative to `scale`, the same sums with every term taken absolute: PI == 0 exactly where the oracle's x is
# NaN or <= 0, |PI^2 - x| <= 1e-9 scale elsewhere.  A column where either side decides a level by rounding is ambiguous
# and left out: a `tr >= tre` test or the `p_lcl > p` test within 1e-9 relative of a tie, or |x| < 1e-9 scale.  The census
# caps their number.  chi = (sps - sp) / (spss - sps) is held to an entropy error of 1e-10 J/kg/K in numerator and
# denominator (about 100 ulp of the 9000 J/kg/K that cp log T and Rd log p reach before they cancel):
# |d chi| <= 2e-10 (1 + |chi|) / |spss - sps|; columns with |spss - sps| < 1 J/kg/K are ambiguous for chi.
PI_BOUND, AMBIGUOUS, CHI_BUDGET, CHI_MIN_DENOM, AMBIGUOUS_SHARE = 1e-9, 1e-9, 2e-10, 1.0, 0.005


def _oracle_columns(tb, cecd, p, sst, psl, T, r):
    """The oracle over [L, n] columns, with what it decided, as arrays."""
    from oracle import thermo_oracle as to
    n = len(sst)
    k_mid = int(np.argmin(np.abs(p - 60000.0)))
    res = [to.potential_intensity(tb, cecd, float(sst[c]), float(psl[c]), p, T[:, c], r[:, c]) for c in range(n)]
    O = {k: np.array([a[k] for _, a in res]) for k in res[0][1]}
    O['pi'] = np.array([v for v, _ in res])
    chi = [to.sat_deficit(float(sst[c]), float(psl[c]), float(T[k_mid, c]), float(p[k_mid]), float(r[k_mid, c])) for c in range(n)]
    O['chi'] = np.array([v for v, _ in chi])
    O['chi_denom'] = np.array([e['spss'] - e['sps'] for _, e in chi])
    O['rh'] = np.array([to.conv_q_to_rh(float(T[k_mid, c]), float(r[k_mid, c]), float(p[k_mid])) for c in range(n)])
    with np.errstate(invalid='ignore'):
        O['amb'] = (O['margin'] < AMBIGUOUS) | (O['lcl_margin'] < AMBIGUOUS) | (np.abs(O['x']) < AMBIGUOUS * O['scale'])
        O['amb_chi'] = np.abs(O['chi_denom']) < CHI_MIN_DENOM
    O['k_mid'] = k_mid
    return O


def _top_rule_shows(O, p):
    """Columns in which the reference's rule 'the top level is on the moist adiabat whatever the LCL' moves x: the LCL above
    the top level, the unsaturated parcel's last hit at the level below with a buoyancy that is not zero, a PI."""
    with np.errstate(invalid='ignore'):
        return ~(O['p_lcl'] > p[-1]) & ~np.isnan(O['p_lcl']) & (O['a_out'] == len(p) - 2) & (O['dT1_a'] != 0) & (O['top_rule'] != 0) & (O['pi'] > 0) & ~O['amb']


def _check_pi(what, pi, O):
    """The rule above; returns the largest |PI^2 - x| / scale."""
    x, scale, ok = O['x'], O['scale'], ~O['amb']
    with np.errstate(invalid='ignore'):
        zero = np.isnan(x) | (x <= 0)
    bad = np.nonzero(ok & ((pi == 0) != zero))[0]
    assert bad.size == 0, '%s: PI == 0 disagrees with the oracle in columns %s' % (what, bad[:10])
    sel = ok & ~zero
    ratio = np.abs(pi[sel] ** 2 - x[sel]) / scale[sel]
    worst = float(ratio.max()) if ratio.size else 0.0
    print('%s: %d columns, %d ambiguous, %d zero, max |PI^2 - x| / scale = %.2e' % (what, pi.size, int((~ok).sum()), int((ok & zero).sum()), worst))
    assert (ratio <= PI_BOUND).all(), '%s: columns %s exceed %g' % (what, np.nonzero(sel)[0][~(ratio <= PI_BOUND)][:10], PI_BOUND)
    return worst


def _check_chi_rh(what, chi, rh, O, chi_ref=None):
    """chi within the entropy budget on the columns that are not ambiguous for it, rh at rtol 1e-12, NaNs alike."""
    ref = O['chi'] if chi_ref is None else chi_ref
    ok = ~O['amb_chi']
    assert np.array_equal(np.isnan(chi), np.isnan(ref))          # ambiguity excuses the size of an error, not a NaN
    sel = ok & ~np.isnan(ref)
    ratio = np.abs(chi[sel] - ref[sel]) * np.abs(O['chi_denom'][sel]) / (1 + np.abs(ref[sel]))
    worst = float(ratio.max()) if ratio.size else 0.0
    print('%s: chi on %d columns, %d ambiguous, max |d chi| |spss - sps| / (1 + |chi|) = %.2e J/kg/K' % (what, chi.size, int((~ok).sum()), worst))
    assert (ratio <= CHI_BUDGET).all()
    np.testing.assert_allclose(rh, O['rh'], rtol=1e-12, atol=0, equal_nan=True)
    return worst


@pytest.fixture(scope='module')
def era5_cases():
    return np.load(os.path.join(GOLDEN, 'thermo_cases_era5.npz'))


@pytest.fixture(scope='module')
def family(table, cases):
    """The 1500-column ERA5 family and the oracle's results on it, computed once and left unchanged."""
    from oracle import thermo_oracle as to
    p = tc.ERA5_LEVELS_PA
    sst, psl, T, r = tc.family(np.random.default_rng(FAMILY_SEED), FAMILY_N, p)
    O = _oracle_columns(to.Table(table['p'], table['s'], table['T']), float(cases['Ck_over_Cd']), p, sst, psl, T, r)
    for a in (sst, psl, T, r) + tuple(v for v in O.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return dict(p=p, sst=sst, psl=psl, T=T, r=r, O=O)


@pytest.fixture(scope='module')
def golden_oracle(table, era5_cases):
    """tag -> the oracle's results on the columns of thermo_cases_era5.npz."""
    from oracle import thermo_oracle as to
    tb = to.Table(table['p'], table['s'], table['T'])
    return {tag: _oracle_columns(tb, float(era5_cases['Ck_over_Cd']), *(era5_cases[tag + '_' + k] for k in ('p', 'sst', 'psl', 'T', 'r')))
            for tag in ('era5',) + tuple(tc.FEW_LEVELS_PA)}


@pytest.mark.parametrize('tag', ['era5', 'l2', 'l3', 'l4'])
def test_oracle_matches_reference_era5_levels(era5_cases, golden_oracle, tag):
    """The oracle against the reference's own outputs on ERA5's 37 non-uniform levels, seven of them above the entropy
    table, and on two, three and four levels; the tolerances of test_oracle_matches_reference."""
    O = golden_oracle[tag]
    assert np.array_equal(era5_cases[tag + '_p'], tc.ERA5_LEVELS_PA if tag == 'era5' else tc.FEW_LEVELS_PA[tag])
    assert O['k_mid'] == int(era5_cases[tag + '_k_mid'])
    np.testing.assert_allclose(O['pi'], era5_cases[tag + '_PI'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(O['chi'], era5_cases[tag + '_chi'], rtol=1e-12, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(O['rh'], era5_cases[tag + '_rh_mid'], rtol=1e-13, atol=0, equal_nan=True)
    assert np.array_equal(O['pi'] == 0, era5_cases[tag + '_PI'] == 0)
    # the columns must say something: enough of them with a PI, and on every axis that has a level between the lowest and
    # the top enough in which the top-level rule moves x (on two levels the level below the top is level 0: dT1 is 0)
    p = era5_cases[tag + '_p']
    shows = _top_rule_shows(O, p)
    print('%s: %d of %d columns with PI > 0, the top-level rule shows in %d' % (tag, int((O['pi'] > 0).sum()), O['pi'].size, int(shows.sum())))
    assert (O['pi'] > 0).sum() >= 16
    assert tag == 'l2' or shows.sum() >= 3


def test_table_lookup_on_nonuniform_knots(table):
    """Table.ev against RectBivariateSpline(kx=1, ky=1).ev on a non-uniform subset of the table's knots: at the knots, at
    random points and outside both axes.  Bound: 4 ulp of the result (the four products are summed in FITPACK's order;
    what is left is the weights' own rounding)."""
    from scipy.interpolate import RectBivariateSpline
    from oracle import thermo_oracle as to
    rng = np.random.default_rng(7)
    p, s, T = tc.subset_table(table['p'], table['s'], table['T'], rng)
    assert p[0] == table['p'][0] and p[-1] == table['p'][-1] and s[0] == table['s'][0] and s[-1] == table['s'][-1]
    assert np.ptp(np.diff(p)) > 0 and np.ptp(np.diff(s)) > 0 and 55 <= len(p) <= 65 and 65 <= len(s) <= 75
    tb, f = to.Table(p, s, T), RectBivariateSpline(p, s, T, kx=1, ky=1)
    P, S = np.meshgrid(p, s, indexing='ij')
    lo, hi = lambda x: x[0] - (x[-1] - x[0]) * rng.uniform(0, 0.5, size=200), lambda x: x[-1] + (x[-1] - x[0]) * rng.uniform(0, 0.5, size=200)
    inside = lambda x: rng.uniform(x[0], x[-1], size=200)
    for what, pp_, ss_ in (('knots', P.ravel(), S.ravel()), ('random points', rng.uniform(p[0], p[-1], size=2000), rng.uniform(s[0], s[-1], size=2000)),
                           ('outside', np.concatenate([lo(p), hi(p), lo(p), hi(p), inside(p), inside(p)]),
                            np.concatenate([lo(s), hi(s), hi(s), lo(s), lo(s), hi(s)]))):
        got, want = np.array([tb.ev(a, b) for a, b in zip(pp_, ss_)]), f.ev(pp_, ss_)
        d = np.abs(got - want)
        print('Table.ev vs RectBivariateSpline.ev, %s: max |d| = %.2e K = %.1f ulp' % (what, d.max(), (d / np.spacing(np.abs(want))).max()))
        assert (d <= 4 * np.spacing(np.abs(want))).all()
    assert np.isnan(tb.ev(np.nan, s[3])) and np.isnan(tb.ev(p[3], np.nan))


def test_family_reaches_every_branch(family, table):
    """The coverage is a condition: the family must reach every branch of the fold often enough to matter, and must not
    lean on columns whose outcome rounding decides."""
    O, p, n = family['O'], family['p'], FAMILY_N
    L = len(p)
    off_axis = lambda s: (s < table['s'][0]) | (s > table['s'][-1])
    with np.errstate(invalid='ignore'):
        counts = [('i_cond == 0', O['i_cond'] == 0, 10), ('i_cond == L-1', O['i_cond'] == L - 1, 10), ('s_out == L-1', O['s_out'] == L - 1, 10),
                  ('runs_a >= 2', O['runs_a'] >= 2, 10), ('runs_s >= 2', O['runs_s'] >= 2, 10), ('pi == 0', O['pi'] == 0, 10),
                  ('s_ns off the entropy axis', off_axis(O['s_ns']), 10), ('s_out above the table', p[O['s_out']] < table['p'][0], 10),
                  ('a_out == L-1', O['a_out'] == L - 1, 3), ('ss off the entropy axis', off_axis(O['ss']), 3),
                  # an index of L-1 is also what a parcel with no hit at all gets (the argmax of an all-False column), which
                  # the fold reaches by another branch: a hit at the top level itself and no hit anywhere are counted apart
                  ('s hit at the top level', (O['s_out'] == L - 1) & (O['runs_s'] > 0), 10), ('no s hit', O['runs_s'] == 0, 10),
                  ('a hit at the top level', (O['a_out'] == L - 1) & (O['runs_a'] > 0), 10), ('no a hit', O['runs_a'] == 0, 3),
                  ('s_out inside the clamped levels', (p[O['s_out']] < table['p'][0]) & (O['s_out'] < L - 1), 3),
                  # the one place where `i_cond == L-1` by default (no level above the LCL) differs from a dry top level: the
                  # parcel's temperature at the top enters x as dT2 of the outflow interpolation from a last hit at L-2
                  ('unsaturated at the top, a_out == L-2, dT1 != 0, PI > 0', _top_rule_shows(O, p), 10)]
    print('census of %d columns (seed %d): ' % (n, FAMILY_SEED) + ', '.join('%s: %d' % (k, int(m.sum())) for k, m, _ in counts))
    with np.errstate(invalid='ignore'):
        print('ambiguous: %d for PI (min margin %.1e, min lcl_margin %.1e, min |x| / scale %.1e), %d for chi'
              % (int(O['amb'].sum()), np.nanmin(O['margin']), np.nanmin(O['lcl_margin']), np.nanmin(np.abs(O['x']) / O['scale']), int(O['amb_chi'].sum())))
    for k, m, need in counts:
        assert int(m.sum()) >= need, k
    assert (p < table['p'][0]).sum() == 7 and np.ptp(np.diff(np.log(p))) > 0.1        # the top seven levels are clamped; the levels are not uniform
    assert O['amb'].sum() <= AMBIGUOUS_SHARE * n
    assert O['amb_chi'].sum() <= AMBIGUOUS_SHARE * n


def _engine(table):
    from tropical_cyclone_risk_amd import preprocess as pp
    from tropical_cyclone_risk_amd.engine import TCEngine
    eng = TCEngine('GL', device=0)
    pp.stage_entropy_table(eng, table['p'], table['s'], table['T'])
    return eng, pp


@pytest.mark.gpu
def test_kernels_match_oracle_on_era5_family(family, table, built_lib):
    """k_potential_intensity / k_chi_rh on the 1500 family columns at ERA5's levels, by the rule above."""
    eng, pp = _engine(table)
    F, O = family, family['O']
    pi = pp.potential_intensity(eng, F['sst'], F['psl'], F['p'], F['T'], F['r'])
    chi, rh = pp.chi_rh(eng, F['sst'], F['psl'], F['T'][O['k_mid']], F['r'][O['k_mid']], float(F['p'][O['k_mid']]))
    eng.close()
    _check_pi('ERA5 family', pi, O)
    _check_chi_rh('ERA5 family', chi, rh, O)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['era5', 'l2', 'l3', 'l4'])
def test_kernels_match_reference_era5_levels(era5_cases, golden_oracle, table, built_lib, tag):
    """The golden columns at ERA5's levels and on two, three and four levels (two is the fewest the ABI takes, and the
    loop then ends on the appended dlnp; of the four, half are above the table): by the rule above against the oracle, and
    against the reference's own PI as test_kernels_match_reference_golden does (same zeros, 1e-9 of max(ref, 1)) wherever
    x >= 0.01 scale, so that the square root does not amplify the error."""
    eng, pp = _engine(table)
    C, O = era5_cases, golden_oracle[tag]
    p, sst, psl, T, r = (C[tag + '_' + k] for k in ('p', 'sst', 'psl', 'T', 'r'))
    pi = pp.potential_intensity(eng, sst, psl, p, T, r)
    chi, rh = pp.chi_rh(eng, sst, psl, T[O['k_mid']], r[O['k_mid']], float(p[O['k_mid']]))
    eng.close()
    _check_pi(tag, pi, O)
    ref = C[tag + '_PI']
    with np.errstate(invalid='ignore'):
        big = ~O['amb'] & (O['x'] >= 0.01 * O['scale'])
    assert np.array_equal(pi[big] == 0, ref[big] == 0)
    err = np.abs(pi[big] - ref[big]) / np.maximum(ref[big], 1.0)
    print('%s: PI vs the reference on %d of %d columns, max rel err %.2e' % (tag, int(big.sum()), pi.size, err.max() if err.size else 0.0))
    assert (err < 1e-9).all()
    _check_chi_rh(tag, chi, rh, O, chi_ref=C[tag + '_chi'])
    np.testing.assert_allclose(rh, C[tag + '_rh_mid'], rtol=1e-12, atol=0, equal_nan=True)


@pytest.mark.gpu
def test_kernels_on_a_nonuniform_table(family, cases, table, built_lib):
    """The entropy table on a non-uniform subset of its knots, where tab_cell's uniform-grid guess is wrong and its two
    walking loops have to move: 512 family columns against the oracle on the same table, by the rule above."""
    from oracle import thermo_oracle as to
    eng, pp = _engine(table)
    F, n = family, 512
    sst, psl, T, r = F['sst'][:n], F['psl'][:n], F['T'][:, :n], F['r'][:, :n]
    full = pp.potential_intensity(eng, sst, psl, F['p'], T, r)
    ps, ss, Ts = tc.subset_table(table['p'], table['s'], table['T'], np.random.default_rng(11))
    O = _oracle_columns(to.Table(ps, ss, Ts), float(cases['Ck_over_Cd']), F['p'], sst, psl, T, r)
    pp.stage_entropy_table(eng, ps, ss, Ts)
    pi = pp.potential_intensity(eng, sst, psl, F['p'], T, r)
    pp.stage_entropy_table(eng, table['p'], table['s'], table['T'])
    again = pp.potential_intensity(eng, sst, psl, F['p'], T, r)
    eng.close()
    _check_pi('non-uniform table', pi, O)
    moved = np.abs(O['x'] - F['O']['x'][:n]) > 1e-6 * O['scale']
    print('non-uniform table: x differs from the full table\'s by more than 1e-6 scale in %d of %d columns' % (int(moved.sum()), n))
    assert moved.sum() > n // 4                        # the coarser table is a different function: the test is not vacuous
    assert np.array_equal(again, full)                 # and the full table is back


@pytest.mark.gpu
def test_launch_edges_and_device_entry(family, cases, table, built_lib):
    """One thread per column, 256 per block: 1, 255, 256, 257 and 1500 columns, and a slice from the far end, give bit
    for bit the matching slices of the full call; tcr_potential_intensity_dev on a side stream equals the host entry."""
    import ctypes as C
    import torch
    eng, pp = _engine(table)
    F = family
    k_mid = F['O']['k_mid']
    call = lambda sl: pp.potential_intensity(eng, F['sst'][sl], F['psl'][sl], F['p'], F['T'][:, sl], F['r'][:, sl])
    call_chi = lambda sl: pp.chi_rh(eng, F['sst'][sl], F['psl'][sl], F['T'][k_mid, sl], F['r'][k_mid, sl], float(F['p'][k_mid]))
    full, (chi, rh) = call(slice(None)), call_chi(slice(None))
    assert full.shape == (FAMILY_N,) and not np.isnan(full).any()
    for sl in [slice(0, n) for n in (1, 255, 256, 257, FAMILY_N)] + [slice(FAMILY_N - 257, FAMILY_N), slice(700, 701)]:
        assert np.array_equal(call(sl), full[sl]), sl
        c2, r2 = call_chi(sl)
        assert np.array_equal(c2, chi[sl], equal_nan=True) and np.array_equal(r2, rh[sl], equal_nan=True), sl
    n = 257
    dev = torch.device('cuda', 0)
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64, order='C'), device=dev)
    dp, dsst, dpsl, dT, dr = t(F['p']), t(F['sst'][:n]), t(F['psl'][:n]), t(F['T'][:, :n]), t(F['r'][:, :n])
    out = torch.full((n + 1,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    eng._ck(eng.L.tcr_potential_intensity_dev(eng.h, n, len(F['p']), dp.data_ptr(), dsst.data_ptr(), dpsl.data_ptr(), dT.data_ptr(),
                                              dr.data_ptr(), float(cases['Ck_over_Cd']),
                                              out.data_ptr(), C.c_void_p(side.cuda_stream)))
    side.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], full[:n]) and got[n] == -1.0        # and nothing past the last column is written
    eng.close()


@pytest.mark.gpu
def test_compute_thermo_host_mirror_era5_levels(family, table, built_lib):
    """compute_thermo with ERA5's 37 levels as the files deliver them, top-down in hPa, against the direct calls on
    bottom-up Pa, bit for bit; the mid level it picks is 600 hPa."""
    eng, pp = _engine(table)
    F, n = family, 384
    p, sst, psl, T, r = F['p'], F['sst'][:n], F['psl'][:n], F['T'][:, :n], F['r'][:, :n]
    k_mid = F['O']['k_mid']
    assert p[k_mid] == 60000.0
    pi = pp.potential_intensity(eng, sst, psl, p, T, r)
    chi, rh = pp.chi_rh(eng, sst, psl, T[k_mid], r[k_mid], 60000.0)
    v2, c2, r2 = pp.compute_thermo(eng, sst, psl, (p / 100)[::-1], 'hPa', T[::-1], r[::-1])
    eng.close()
    # ERA5's levels are whole hPa: (p / 100) * 100 is p bit for bit, the kernels see the same inputs, the results are equal
    assert np.array_equal((p / 100) * 100, p)
    assert np.array_equal(v2, pi) and np.array_equal(r2, rh, equal_nan=True)
    assert np.array_equal(c2, np.minimum(np.maximum(chi, 0), 10), equal_nan=True)
    # rh at 600 hPa is what came back, and no neighbouring level gives it
    for k in (k_mid - 1, k_mid + 1):
        from oracle import thermo_oracle as to
        other = np.array([to.conv_q_to_rh(float(T[k, c]), float(r[k, c]), float(p[k])) for c in range(n)])
        assert not np.allclose(other, r2, rtol=1e-6, equal_nan=True)
