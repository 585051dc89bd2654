"""Directional wind (include/tcrisk_hip.h "directional wind", tropical_cyclone_risk_amd/directional.py, csrc/tcr_directional.hip):
hand values of the NumPy restatement (tests/directional_numpy.py), the argument handling and the command line without a GPU; on
the GPU the restatement's rule for the planes, counts from the call's own planes, exact agreement with the wind footprint, the
sector algebra, bit-identity, the entry points and the command line."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import directional_numpy as RN
from tests import levels_numpy as LN
from tests import windfield_numpy as WN
from tests.test_duration import _sites, _tracks

DT = 3600.0


# ------------------------------------------------------------------------------------------------------------------ CPU
def _line_track(n, lat0=20.0, v0=30.0):
    """One storm of n samples moving west along lat0, a quarter of a degree per hour, and a calm environment."""
    lon = (290.0 - 0.25 * np.arange(n))[None, :]
    lat = np.full((1, n), lat0)
    v = np.full((1, n), v0)
    env = [np.zeros((1, n)) for _ in range(4)]
    return lon, lat, v, env


def _pair(rec, q, slon, slat):
    """(from-bearing, |w|) of record q of one storm's records at one site."""
    we, wn, w, _ = RN.wind_vector(slon, slat, *[x[q] for x in rec], 1.0)
    return float(RN.from_deg(we, wn)), float(w)


def test_restatement_hand_values():
    n = 9
    for lat0, north, south in ((20.0, 90.0, 270.0), (-20.0, 270.0, 90.0), (0.0, 90.0, 270.0), (-1e-6, 270.0, 90.0)):
        lon, lat, v, env = _line_track(n, lat0)
        rec = WN.samples(lon, lat, v, env, DT)[0]
        # cyclonic flow plus a westward asymmetry: due north of a centre in the north the wind is an easterly, exactly
        th, w = _pair(rec, 4, lon[0, 4], lat0 + 0.6)
        assert th == north and w > 1.0, (lat0, th)
        th, w = _pair(rec, 4, lon[0, 4], lat0 - 0.6)
        assert th == south and w > 1.0, (lat0, th)
        assert _pair(rec, 4, lon[0, 4], lat0)[1] == 0.0                 # a site on the centre: no wind, no sector
    assert RN.sector_of(90.0, 8, 0.0)[0] == 2 and RN.sector_of(270.0, 8, 0.0)[0] == 6 and RN.sector_of(359.0, 8, 0.0)[0] == 0
    assert RN.sector_of(22.4, 8, 0.0) == (0, -1) and RN.sector_of(22.5, 8, 0.0) == (1, 0) and RN.sector_of(350.0, 1, 0.0) == (0, -1)
    assert RN.sector_of(10.0, 5, 10.0)[0] == 0 and RN.sector_of(333.9, 5, 10.0)[0] == 4 and RN.sector_of(334.1, 5, 10.0)[0] == 0

    # one storm, one sample's worth of geometry: sites due north and due south of sample 4, and one on it
    lon, lat, v, env = _line_track(n)
    recs = WN.samples(lon, lat, v, env, DT)
    slon, slat = np.array([lon[0, 4], lon[0, 4], lon[0, 4]]), np.array([20.6, 19.4, 20.0])
    lo, amb, inc_any, inc_sure = RN.directional(recs, slon, slat, 500.0, 1.0, 8, 0.0)
    assert lo.shape == (8, 3, 1) and not amb and inc_any.all() and inc_sure.all() and not np.isnan(lo).any()
    w_all = WN.site_max(recs, slon, slat, 500.0, 1.0)[0]
    assert np.array_equal(lo.max(axis=0), w_all)                        # the sectors' maximum is the footprint's
    assert lo[2, 0, 0] >= _pair(recs[0], 4, slon[0], slat[0])[1] and lo[6, 1, 0] >= _pair(recs[0], 4, slon[1], slat[1])[1]
    # with the boundaries on the axes those exactly-90 and exactly-270 pairs can go either way
    lo4, amb4, _, _ = RN.directional(recs, slon, slat, 500.0, 1.0, 4, 45.0)
    assert set(amb4) == {(0, 0), (1, 0)}
    for (i, _), (winds, may) in amb4.items():
        assert winds.tolist() == [_pair(recs[0], 4, slon[i], slat[i])[1]]
        assert may.tolist() == ([[True, True, False, False]] if i == 0 else [[False, False, True, True]])
    # far to the north of the whole track every wind is an easterly of some kind: 0.0 elsewhere, not NaN
    lo1, amb1, any1, sure1 = RN.directional(recs, np.array([289.0]), np.array([22.0]), 500.0, 1.0, 8, 0.0)
    assert not amb1 and sure1.all() and lo1[:, 0, 0].tolist()[4:] == [0.0] * 4 and lo1[0, 0, 0] == 0.0 and lo1[2, 0, 0] > 1.0
    # out of reach: NaN in every sector; and a one-sample track has no records
    lo2, _, any2, _ = RN.directional(recs, np.array([200.0]), np.array([-30.0]), 500.0, 1.0, 8, 0.0)
    assert not any2.any() and np.isnan(lo2).all()
    lon1 = lon.copy()
    lon1[0, 1] = np.nan
    recs1 = WN.samples(lon1, lat, v, env, DT)
    assert recs1[0] is None and np.isnan(RN.directional(recs1, slon, slat, 500.0, 1.0, 8, 0.0)[0]).all()
    # counts of the restatement's own planes
    c = RN.counts(lo, np.zeros(1, int), 2, [0.5, 1e3])
    assert c.shape == (3, 2, 8, 2) and c[0, 0, 2].tolist() == [1, 0] and not c[:, 1].any()
    # the rule: lo itself passes, a NaN where a pair is surely included does not, nor a wrong value
    assert RN.allowed(lo, lo, amb, inc_any, inc_sure).all()
    bad = lo.copy()
    bad[3, 0, 0] = np.nan
    assert not RN.allowed(bad, lo, amb, inc_any, inc_sure)[:, 0, 0].any()
    bad = lo.copy()
    bad[2, 0, 0] *= 1.0 + 1e-9
    assert not RN.allowed(bad, lo, amb, inc_any, inc_sure)[2, 0, 0]
    # an ambiguous pair may be in either of its sectors, and in no other
    w0 = amb4[(0, 0)][0][0]
    for j, ok in ((0, True), (1, True), (2, False)):
        got = lo4.copy()
        if w0 > got[j, 0, 0]:
            got[j, 0, 0] = w0
            assert RN.allowed(got, lo4, amb4, inc_any, inc_sure)[j, 0, 0] == ok, j


def test_defaults():
    from tropical_cyclone_risk_amd import directional
    assert directional.DEFAULT_THRESHOLDS.tolist() == [10, 20, 30, 40, 50, 60, 70]
    assert directional.sector_centres(8).tolist() == [0, 45, 90, 135, 180, 225, 270, 315]
    assert directional.sector_centres(4, 300.0).tolist() == [300, 30, 120, 210]
    c = np.zeros((2, 3, 4, 2), np.int32)
    c[0, 0, 1] = [3, 1]
    c[0, 2, 3] = [5, 2]
    assert directional.return_periods(c, 6).tolist()[0] == [[np.inf, np.inf], [2.0, 6.0], [np.inf, np.inf], [1.2, 3.0]]
    assert directional.worst_sector(c, 6) == [(3, 1, 3.0), (-1, -1, np.inf)]


def test_argument_errors_before_any_device_work():
    from tropical_cyclone_risk_amd import directional
    rng = np.random.default_rng(0)
    lon, lat, v = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    env = [np.zeros((3, 5))] * 4
    base = dict(lon=lon, lat=lat, v=v, env=env, groups=np.zeros(3, np.int64), site_lon=np.array([280.0]), site_lat=np.array([20.0]),
                dt_s=DT)
    bad = [dict(n_sector=0), dict(n_sector=9), dict(n_sector=2.5), dict(n_sector=True),
           dict(sector0_deg=360.0), dict(sector0_deg=-1.0), dict(sector0_deg=np.nan), dict(sector0_deg=np.inf),
           dict(n_sector=8, thresholds=np.arange(1.0, 9.0)),                          # 8 * 9 = 72 cells
           dict(n_sector=3, thresholds=np.arange(1.0, 23.0)),                         # 3 * 22 = 66 cells
           dict(thresholds=np.arange(10.0, 81.0, 5.0)),                               # the footprint's 15 with the default 8 sectors
           dict(thresholds=[3.0, 1.0]), dict(thresholds=[]), dict(thresholds=[1.0, np.inf]), dict(thresholds=[1.0, 1.0]),
           dict(return_max=[8]), dict(return_max=[0, 0]), dict(return_max='x'), dict(n_sector=4, return_max=[4]),
           # the footprint's own rules
           dict(r_out_km=0.0), dict(r_out_km=2000.5), dict(substeps=0), dict(substeps=65), dict(substeps=1.5), dict(ck_cd=2.0),
           dict(dt_s=0.0), dict(rmax_km=-5.0), dict(rmax_km=np.full((3, 4), 20.0)), dict(env=env[:3]), dict(v=v[:, :4]),
           dict(groups=np.zeros(2, np.int64)), dict(site_lat=np.array([np.nan])), dict(groups=np.array([0, 1, 2]), n_groups=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            directional.site_directional_wind(**dict(base, **kw))
    # the limit itself passes the checks: 8 * 8 and 1 * 64 cells
    assert directional._check_sectors(8, 0.0, np.arange(1.0, 8.0), True) == (8, 0.0, list(range(8)))
    assert directional._check_sectors(1, 359.5, np.arange(1.0, 64.0), [0]) == (1, 359.5, [0])


def test_cli_arguments(capsys):
    from tropical_cyclone_risk_amd import directional
    a = directional.parse_args(['x.nc', '--site', '1,2'])
    assert a.sectors == 8 and a.sector0_deg == 0.0 and np.array_equal(a.thresholds, directional.DEFAULT_THRESHOLDS)
    assert a.r_out_km == 500.0 and a.substeps == 1 and a.rmax_km is None and a.ck_cd is None and a.out == 'directional.npz'
    assert a.return_periods is None
    b = directional.parse_args(['x.nc', '--grid', '270:271:0.5,20:21:1', '--sectors', '4', '--sector0-deg', '45', '--thresholds',
                                '10:50:10', '--r-out-km', '300', '--substeps', '4', '--return-periods', '10,50'])
    assert b.sectors == 4 and b.sector0_deg == 45.0 and b.thresholds.tolist() == [10, 20, 30, 40, 50] and b.substeps == 4
    assert list(b.return_periods) == [10.0, 50.0]
    assert directional.parse_args(['x.nc', '--site', '1,2', '--thresholds', '12.5,20,33']).thresholds.tolist() == [12.5, 20.0, 33.0]
    for argv in (['x.nc'], ['x.nc', '--site', '1,2', '--sectors', '9'], ['x.nc', '--site', '1,2', '--sectors', '0'],
                 ['x.nc', '--site', '1,2', '--sector0-deg', '360'], ['x.nc', '--site', '1,2', '--thresholds', '10:80:5'],
                 ['x.nc', '--site', '1,2', '--thresholds', 'a,b'],
                 ['x.nc', '--site', '1,2', '--return-periods', '10', '--tail-exceedances', '5']):
        with pytest.raises(SystemExit):
            directional.parse_args(argv)
    assert 'not offered' in capsys.readouterr().err


def test_directional_symbols_exported(built_lib):
    from tropical_cyclone_risk_amd import _lib
    assert os.path.samefile(built_lib, _lib.LIB_PATH)
    L = _lib.lib()                                                      # (the package's own way in: one HIP runtime per process)
    for name in ('tcr_directional_dev', 'tcr_directional_host', 'tcr_directional_pairs'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.tcr_abi_version() == 7


# substeps, ck_cd, rm (None: Willoughby, a constant, 'plane'), r_out, n_sector, sector0_deg
CASES = [(1, 1.0, None, 500.0, 8, 0.0),
         (3, 0.5, 35.0, 300.0, 4, 45.0),
         (6, 1.5, 'plane', 150.0, 1, 0.0),
         (3, 1.0, 'plane', 800.0, 8, 22.5),
         (2, 1.0, None, 500.0, 5, 10.0)]
# thresholds per n_sector: 8 * 8 = 64 cells, the limit; the footprint's own 15 for the one-sector case
THRESHOLDS = {8: np.linspace(8.0, 50.0, 7), 4: np.linspace(8.0, 50.0, 15), 1: np.arange(10.0, 81.0, 5.0), 5: np.linspace(8.0, 50.0, 11)}


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs of CASES[i] and the restatement on them (computed once, never changed)."""
    sub, c, rm, r_out, n_sector, sector0 = CASES[i]
    rng, lon, lat, v, env, groups, n_groups = _tracks(300 + i)
    if isinstance(rm, str):
        rm = rng.uniform(8.0, 90.0, lon.shape)
    slon, slat = _sites(rng, lon, lat, r_out)
    recs = WN.samples(lon, lat, v, env, DT, rmax_km=rm, substeps=sub)
    lo, amb, inc_any, inc_sure = RN.directional(recs, slon, slat, r_out, c, n_sector, sector0)
    for a in (lo, inc_any, inc_sure):
        a.setflags(write=False)
    kw = dict(n_sector=n_sector, sector0_deg=sector0, thresholds=THRESHOLDS[n_sector], rmax_km=rm, ck_cd=c, r_out_km=r_out,
              substeps=sub, n_groups=n_groups)
    return dict(tracks=(lon, lat, v, env, groups), sites=(slon, slat), kw=kw, ref=(lo, amb, inc_any, inc_sure), n_groups=n_groups)


def _condition(ref):
    """What makes a case a test: (share of the possibly included cells without an ambiguous pair, per sector the cells without
    one whose peak is above 10 m/s)."""
    lo, amb, inc_any, _ = ref
    exact = inc_any & ~RN.ambiguous_cells(amb, inc_any.shape)
    with np.errstate(invalid='ignore'):
        return exact.sum() / inc_any.sum(), [int((exact & (lo[k] > 10.0)).sum()) for k in range(lo.shape[0])]


@pytest.mark.parametrize('i', range(len(CASES)))
def test_cases_are_decided_by_the_restatement(i):
    """Not a measurement: the cases are chosen so that nearly every cell has one allowed answer, and every sector is blown from."""
    share, reached = _condition(_case(i)['ref'])
    print('case %d: %.4f of the cells exact, exact cells above 10 m/s per sector %s' % (i, share, reached))
    assert share >= 0.95 and min(reached) >= 50
    assert _case(i)['sites'][0].size % 64 != 0


# ------------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _gpu(i):
    from tropical_cyclone_risk_amd import directional
    d = _case(i)
    lon, lat, v, env, groups = d['tracks']
    return directional.site_directional_wind(lon, lat, v, env, groups, d['sites'][0], d['sites'][1], DT, return_max=True, **d['kw'])


def _footprint(i, **more):
    from tropical_cyclone_risk_amd import windfield
    d = _case(i)
    lon, lat, v, env, groups = d['tracks']
    kw = {k: d['kw'][k] for k in ('rmax_km', 'ck_cd', 'r_out_km', 'substeps', 'n_groups')}
    return windfield.site_wind(lon, lat, v, env, groups, d['sites'][0], d['sites'][1], DT, return_max=True, **dict(kw, **more))


def _fmax(planes):
    """The maximum over the first axis that skips NaN only where another value is there: fmax, which moves no bits."""
    out = planes[0]
    for p in planes[1:]:
        out = np.fmax(out, p)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(CASES)))
def test_gpu_matches_restatement(built_lib, i):
    d, r = _case(i), _gpu(i)
    lo, amb, inc_any, inc_sure = d['ref']
    share, reached = _condition(d['ref'])
    assert share >= 0.95 and min(reached) >= 50
    m = r['site_dir_max']
    assert m.shape == lo.shape and np.array_equal(r['sector_from_deg'], (CASES[i][5] + np.arange(CASES[i][4]) * 360.0 / CASES[i][4]) % 360)
    nan = np.isnan(m)
    assert (nan == nan[0]).all()                                        # NaN is the same in every sector
    assert not (nan[0] & inc_sure).any() and not (~nan[0] & ~inc_any).any()
    assert (m[~nan] >= 0).all()
    ok = RN.allowed(m, lo, amb, inc_any, inc_sure)
    worst = [(int(k), int(a), int(s), float(m[k, a, s]), float(lo[k, a, s])) for k, a, s in np.argwhere(~ok)[:5]]
    print('case %d: %d cells, %d not allowed %s' % (i, ok.size, int((~ok).sum()), worst))
    assert ok.all(), worst
    exact = np.broadcast_to(~RN.ambiguous_cells(amb, inc_any.shape), m.shape)
    assert WN.close(m[exact], lo[exact]).all()                          # no ambiguous pair: lo, full stop
    assert np.isnan(m[:, :, :5]).all()                                  # one-sample tracks


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(CASES)))
def test_gpu_counts_from_own_planes(built_lib, i):
    d, r = _case(i), _gpu(i)
    groups, n_groups = d['tracks'][4], d['n_groups']
    n_sector, thr = CASES[i][4], d['kw']['thresholds']
    assert r['counts'].dtype == np.int32 and r['counts'].shape == (d['sites'][0].size, n_groups, n_sector, thr.size)
    assert np.array_equal(r['thresholds'], thr)
    assert np.array_equal(r['counts'], RN.counts(r['site_dir_max'], groups, n_groups, thr))
    assert r['counts'].sum() > 100 and (np.diff(r['counts'], axis=3) <= 0).all()
    assert r['counts'].sum(axis=(0, 1, 3)).min() > 0                    # every sector is blown from
    for g in (1, 4):                                                    # the empty groups
        assert not r['counts'][:, g].any()


@pytest.mark.gpu
def test_gpu_is_the_footprint_exactly(built_lib):
    import types
    from tropical_cyclone_risk_amd import _lib, directional, windfield
    for i in range(len(CASES)):
        r, w = _gpu(i), _footprint(i)
        assert LN.same_bits(_fmax(r['site_dir_max']), w['site_max']), i      # NaN pattern included
    # one sector: the plane is site_max and the counts are the footprint's
    r, w = _gpu(2), _footprint(2, thresholds=THRESHOLDS[1])
    assert LN.same_bits(r['site_dir_max'][0], w['site_max']) and np.array_equal(r['counts'][:, :, 0], w['counts'])
    assert w['counts'].sum() > 100
    # the same pairs are evaluated: both calls on one context, each with a workspace of its own
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        d = _case(0)
        lon, lat, v, env, groups = d['tracks']
        eng = types.SimpleNamespace(h=h)
        a = directional.site_directional_wind(lon, lat, v, env, groups, d['sites'][0], d['sites'][1], DT, engine=eng, **d['kw'])
        kw = {k: d['kw'][k] for k in ('rmax_km', 'ck_cd', 'r_out_km', 'substeps', 'n_groups')}
        windfield.site_wind(lon, lat, v, env, groups, d['sites'][0], d['sites'][1], DT, engine=eng, **kw)
        pd, pw = ctypes.c_int64(), ctypes.c_int64()
        assert L.tcr_directional_pairs(h, ctypes.byref(pd)) == 0 and L.tcr_windfield_pairs(h, ctypes.byref(pw)) == 0
        assert pd.value == pw.value > 0
        assert np.array_equal(a['counts'], _gpu(0)['counts'])
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_sector_algebra(built_lib):
    from tropical_cyclone_risk_amd import directional
    d, r8 = _case(0), _gpu(0)                                           # 8 sectors at 0
    lo, amb, inc_any, _ = d['ref']
    lon, lat, v, env, groups = d['tracks']
    exact = ~RN.ambiguous_cells(amb, inc_any.shape)                     # no pair near one of the 8 boundaries, which hold the 4
    assert exact.sum() > 0.95 * exact.size
    m8 = r8['site_dir_max']
    run = lambda **kw: directional.site_directional_wind(lon, lat, v, env, groups, d['sites'][0], d['sites'][1], DT, return_max=True,
                                                         **dict(d['kw'], **kw))['site_dir_max']          # noqa: E731
    # sector k of 4 at 22.5 degrees is [-22.5 + 90 k, 67.5 + 90 k): the sectors 2 k and 2 k + 1 of 8
    m4 = run(n_sector=4, sector0_deg=22.5)
    for k in range(4):
        assert LN.same_bits(m4[k][exact], np.fmax(m8[2 * k], m8[2 * k + 1])[exact]), k
    # 8 sectors at 45 degrees: the same boundaries, numbered one later
    m45 = run(sector0_deg=45.0)
    for k in range(8):
        assert LN.same_bits(m45[k][exact], m8[(k + 1) % 8][exact]), k
    assert (m8[:, exact] > 10.0).sum(axis=1).min() >= 50


@pytest.mark.gpu
def test_gpu_bit_identical_across_runs_site_order_and_storm_order(built_lib):
    from tropical_cyclone_risk_amd import directional
    d, a = _case(3), _gpu(3)
    lon, lat, v, env, groups = d['tracks']
    slon, slat = d['sites']
    rng = np.random.default_rng(5)
    kw = dict(d['kw'], return_max=True)

    def same(x, y, sites=slice(None), storms=slice(None)):
        assert np.array_equal(x['site_dir_max'].view(np.int64), y['site_dir_max'][:, sites][:, :, storms].view(np.int64))
        assert np.array_equal(x['counts'], y['counts'][sites])
    same(directional.site_directional_wind(lon, lat, v, env, groups, slon, slat, DT, **kw), a)
    ps = rng.permutation(slon.size)
    same(directional.site_directional_wind(lon, lat, v, env, groups, slon[ps], slat[ps], DT, **kw), a, sites=ps)
    pt = rng.permutation(lon.shape[0])                                  # storms shuffled within and across groups
    rm = kw['rmax_km'][pt]
    same(directional.site_directional_wind(lon[pt], lat[pt], v[pt], [e[pt] for e in env], groups[pt], slon, slat, DT,
                                           **dict(kw, rmax_km=rm)), a, storms=pt)


@pytest.mark.gpu
def test_gpu_host_and_device_entry_points_agree(built_lib):
    import types
    import torch
    from tropical_cyclone_risk_amd import _lib, directional
    d, ref = _case(3), _gpu(3)
    lon, lat, v, env, groups = d['tracks']
    slon, slat = d['sites']
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(x, device=dev) for x in [lon, lat, v] + env + [slon, slat, d['kw']['rmax_km']]]
    h = ctypes.c_void_p()
    assert _lib.lib().tcr_ctx_create(0, ctypes.byref(h)) == 0
    eng = types.SimpleNamespace(h=h)                                    # one context, so one workspace, for the three calls
    side = torch.cuda.Stream(dev)
    try:
        for want in (True, [0], False):
            with torch.cuda.stream(side):
                r = directional.site_directional_wind(t[0], t[1], t[2], t[3:7], groups, t[7], t[8], DT, engine=eng, return_max=want,
                                                      **dict(d['kw'], rmax_km=t[9]))
            side.synchronize()
            assert r['counts'].device == dev
            assert np.array_equal(r['counts'].cpu().numpy(), ref['counts'])
            if want is True:
                assert LN.same_bits(r['site_dir_max'].cpu().numpy(), ref['site_dir_max'])
            elif want is not False:
                got = r['site_dir_max'].cpu().numpy()
                assert LN.same_bits(got[0], ref['site_dir_max'][0]) and np.isnan(got[1:]).all()
            else:
                assert 'site_dir_max' not in r
    finally:
        side.synchronize()
        _lib.lib().tcr_ctx_destroy(h)
    # planes for some of the sectors only: the others are NaN, and nothing else moves
    d1, full = _case(1), _gpu(1)
    lon, lat, v, env, groups = d1['tracks']
    part = directional.site_directional_wind(lon, lat, v, env, groups, d1['sites'][0], d1['sites'][1], DT, return_max=[3, 1], **d1['kw'])
    for k in range(4):
        assert LN.same_bits(part['site_dir_max'][k], full['site_dir_max'][k]) if k in (1, 3) else np.isnan(part['site_dir_max'][k]).all()
    assert np.array_equal(part['counts'], full['counts'])
    # no storms at all
    e = directional.site_directional_wind(lon[:0], lat[:0], v[:0], [x[:0] for x in env], groups[:0], d1['sites'][0], d1['sites'][1], DT,
                                          return_max=True, **dict(d1['kw'], n_groups=2, rmax_km=35.0))
    assert e['site_dir_max'].shape == (4, d1['sites'][0].size, 0) and e['counts'].shape == (d1['sites'][0].size, 2, 4, 15)
    assert not e['counts'].any()


@pytest.mark.gpu
def test_gpu_abi_outputs_optional_bad_arguments_and_pairs(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        n_trk, n_t, n_site = 3, 9, 2
        planes = [np.full((n_trk, n_t), x) for x in (280.0, 20.0, 30.0, 1.0, 1.0, 0.0, 0.0)]
        planes[0] = planes[0] - 0.25 * np.arange(n_t) + 0.5 * np.arange(n_trk)[:, None]
        planes[2][2, 4:] = np.nan                                       # a track of four samples
        off = (ctypes.c_int64 * 3)(0, 2, n_trk)
        slon, slat = np.array([279.5, 281.0]), np.array([20.5, 19.6])
        thr0 = np.array([1.0, 15.0, 25.0])
        trk = _lib.WindTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=planes[0].ctypes.data, lat=planes[1].ctypes.data,
                              v=planes[2].ctypes.data, u250=planes[3].ctypes.data, v250=planes[4].ctypes.data,
                              u850=planes[5].ctypes.data, v850=planes[6].ctypes.data, rmax_km=None, n_group=2, group_off=off)

        def call(n_sector=4, sector0=0.0, thr=thr0, rows=None, no_array=False, **p):
            prm = _lib.WindParams(**dict(dict(dt_s=DT, ck_cd=1.0, r_out_km=500.0, rmax_const_km=0.0, substeps=2), **p))
            n_bin, n_row = len(thr), max(min(n_sector, 8), 1)
            counts = np.full((n_site, 2, n_row, max(n_bin, 1)), -7, np.int32)
            dm = np.full((n_row, n_site, n_trk), -7.0)
            arr = (ctypes.c_void_p * n_row)()
            for k in range(n_row) if rows is None else rows:
                arr[k] = dm[k].ctypes.data
            th = np.asarray(thr, float)
            rc = L.tcr_directional_host(h, ctypes.byref(trk), ctypes.byref(prm), n_site, slon.ctypes.data, slat.ctypes.data, n_sector,
                                        sector0, n_bin, th.ctypes.data_as(_lib.DP), counts.ctypes.data, None if no_array else arr)
            return rc, counts, dm
        rc, counts, dm = call()
        assert rc == 0 and counts.sum() > 0 and (counts >= 0).all() and (dm >= 0).all() and dm.max() > 15.0
        assert np.array_equal(counts, RN.counts(dm, np.array([0, 0, 1]), 2, thr0))
        pairs, wpairs = ctypes.c_int64(), ctypes.c_int64()
        assert L.tcr_directional_pairs(h, ctypes.byref(pairs)) == 0 and pairs.value > 0
        # outputs left out: the others are what they were, and nothing is written where nothing was asked for
        for kw in (dict(rows=(1,)), dict(rows=(0, 3)), dict(rows=()), dict(no_array=True)):
            rc, c2, d2 = call(**kw)
            assert rc == 0 and np.array_equal(c2, counts), kw
            for k in range(4):
                assert np.array_equal(d2[k], dm[k]) if (k in kw.get('rows', ()) and not kw.get('no_array')) else (d2[k] == -7).all()
        # the footprint evaluates the same pairs, and its peak is the sectors' maximum
        wc = np.zeros((n_site, 2, 3), np.int32)
        wm = np.zeros((n_site, n_trk))
        prm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=500.0, rmax_const_km=0.0, substeps=2)
        assert L.tcr_windfield_host(h, ctypes.byref(trk), ctypes.byref(prm), n_site, slon.ctypes.data, slat.ctypes.data, 3,
                                    thr0.ctypes.data_as(_lib.DP), wc.ctypes.data, wm.ctypes.data) == 0
        assert L.tcr_windfield_pairs(h, ctypes.byref(wpairs)) == 0 and wpairs.value == pairs.value
        assert LN.same_bits(dm.max(axis=0), wm)
        bad = [dict(n_sector=0), dict(n_sector=9), dict(n_sector=-1), dict(sector0=360.0), dict(sector0=-1.0), dict(sector0=np.nan),
               dict(sector0=np.inf), dict(thr=[3.0, 1.0]), dict(thr=[1.0, np.nan]), dict(thr=[]),
               dict(n_sector=3, thr=np.arange(1.0, 23.0)), dict(n_sector=8, thr=np.arange(1.0, 9.0), rows=()),
               dict(r_out_km=2001.0), dict(substeps=65), dict(ck_cd=2.0), dict(dt_s=0.0), dict(rmax_const_km=-1.0)]
        for kw in bad:
            assert call(**kw)[0] == -1, kw
            assert L.tcr_last_error(h).startswith(b'tcr_directional:'), (kw, L.tcr_last_error(h))
        assert call(n_sector=8, thr=np.arange(1.0, 8.0), rows=())[0] == 0      # 64 cells
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_cli_round_trip(built_lib, tmp_path, capsys):
    from tests.test_levels import _write_track_file
    from tropical_cyclone_risk_amd import analysis, directional, levels
    fn = _write_track_file(tmp_path, np.random.default_rng(5))
    sites = ['--site=-75.0,24.0', '--site', '286.5,25.5', '--site=-72.25,27.0', '--site', '10.0,50.0']
    opts = ['--sectors', '4', '--sector0-deg', '30', '--thresholds', '5:35:10', '--substeps', '2']
    keys = {'counts', 'return_period', 'sector_from_deg', 'thresholds', 'site_lon', 'site_lat', 'total_years', 'r_out_km', 'substeps',
            'rmax_km', 'dt_s', 'group_file', 'group_year', 'files'}
    out = str(tmp_path / 'directional.npz')
    assert directional.main([fn, '--out', out] + sites + opts) == 0
    plain = np.load(out)
    assert set(plain.files) == keys
    text = capsys.readouterr().out
    assert 'worst sector' in text and 'no sector reaches' in text
    lon, lat, vmax, v, env, groups, gfile, gyear, dt = analysis.load_wind_planes([fn])
    api = directional.site_directional_wind(lon, lat, v, env, groups, plain['site_lon'], plain['site_lat'], dt, n_sector=4,
                                            sector0_deg=30.0, thresholds=[5.0, 15.0, 25.0, 35.0], substeps=2, n_groups=3, return_max=True)
    assert int(plain['total_years']) == 3 and float(plain['dt_s']) == dt and plain['sector_from_deg'].tolist() == [30.0, 120.0, 210.0, 300.0]
    assert plain['thresholds'].tolist() == [5.0, 15.0, 25.0, 35.0]
    assert np.array_equal(plain['counts'], api['counts']) and api['counts'].sum() > 0 and plain['counts'].shape == (4, 3, 4, 4)
    assert np.array_equal(plain['return_period'], directional.return_periods(api['counts'], 3))
    assert plain['return_period'].shape == (4, 4, 4) and np.isinf(plain['return_period'][3]).all()
    assert np.isfinite(plain['return_period'][:3, :, 0]).any(axis=1).all()
    assert directional.main([fn, '--out', out, '--return-periods', '2,5'] + sites + opts) == 0
    z = np.load(out)
    assert set(z.files) == keys | {'return_level', 'return_periods', 'n_reach'}
    for name in keys:
        assert np.all((z[name] == plain[name]) | ((z[name] != z[name]) & (plain[name] != plain[name]))), name
    k, ok = levels.ranks_of_periods([2.0, 5.0], 3)
    assert z['return_level'].shape == (4, 4, 2) and np.array_equal(z['return_periods'], [2.0, 5.0])
    for j in range(4):
        want, n_reach = LN.row_select(api['site_dir_max'][j], k)
        want[:, ~ok] = np.nan
        assert LN.same_bits(z['return_level'][:, j], want) and np.array_equal(z['n_reach'], n_reach)
    assert not np.isnan(z['return_level'][:3, :, 0]).any() and np.isnan(z['return_level'][3]).all()
