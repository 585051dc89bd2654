"""Wind duration (include/tcrisk_hip.h "wind duration", tropical_cyclone_risk_amd/duration.py, csrc/tcr_duration.hip): hand values
of the NumPy restatement (tests/duration_numpy.py), the argument handling and the command line without a GPU; on the GPU the
restatement's bounds, counts and totals from the call's own planes, exact agreement with the wind footprint, bit-identity, the
entry points and the command line."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import duration_numpy as DN
from tests import levels_numpy as LN
from tests import windfield_numpy as WN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 3600.0


# ------------------------------------------------------------------------------------------------------------------ CPU
def _line_track(n, v0=30.0):
    """One storm of n samples moving west along 20 N, a quarter of a degree per hour, and a calm environment."""
    lon = (290.0 - 0.25 * np.arange(n))[None, :]
    lat = np.full((1, n), 20.0)
    v = np.full((1, n), v0)
    env = [np.zeros((1, n)) for _ in range(4)]
    return lon, lat, v, env


def test_restatement_hand_values():
    n, sub = 9, 4
    u = DN.unit_hours(DT, sub)
    assert u == 0.125
    lon, lat, v, env = _line_track(n)
    recs = WN.samples(lon, lat, v, env, DT, substeps=sub)
    n_rec = (n - 1) * sub + 1
    assert recs[0].shape[1] == n_rec and DN.half_weights(n_rec).sum() == 2 * (n_rec - 1)
    # a site within r_out of every record and off every centre: every record blows there, however little
    slon, slat = np.array([289.0]), np.array([20.6])
    w, r = WN.wind(slon[:, None], slat[:, None], *[x[None, :] for x in recs[0]], 1.0)
    assert r.max() < 400.0 and r.min() > 30.0 and w.min() > 1.0
    _, _, fac, mag = WN.asymmetry(lon[0], lat[0], v[0], [e[0] for e in env], DT)
    top = float((v[0] + fac * mag).max())
    levels = np.array([1e-300, 10.0, 20.0, 30.0, top + 1.0])
    lo, hi, n_amb, inc_any, inc_sure = DN.duration(recs, slon, slat, 500.0, 1.0, levels)
    assert np.array_equal(lo, hi) and not n_amb.any() and inc_any.all() and inc_sure.all()
    assert lo[0, 0, 0] == 2 * (n_rec - 1)
    h = DN.hours(lo, inc_any, u)
    assert h[0, 0, 0] == n - 1                                          # the weights add up to the track's length, exactly
    assert h[-1, 0, 0] == 0.0                                           # above v + fac |U|: no hours, but not NaN
    assert (np.diff(h[:, 0, 0]) <= 0).all() and 0 < h[2, 0, 0] < h[1, 0, 0] <= n - 1
    # out of reach: NaN at every level; and a one-sample track has no records
    lo2, _, _, any2, _ = DN.duration(recs, np.array([200.0]), np.array([-30.0]), 500.0, 1.0, levels)
    assert not any2.any() and np.isnan(DN.hours(lo2, any2, u)).all()
    lon1 = lon.copy()
    lon1[0, 1] = np.nan
    recs1 = WN.samples(lon1, lat, v, env, DT, substeps=sub)
    assert recs1[0] is None
    lo1, hi1, _, any1, _ = DN.duration(recs1, slon, slat, 500.0, 1.0, levels)
    assert not any1.any() and not hi1.any() and np.isnan(DN.hours(lo1, any1, u)).all()
    # counts and totals of the restatement's own planes
    c = DN.counts(h, np.zeros(1, int), 2, [0.5, float(n - 1), float(n)])
    assert c.shape == (1, 2, 5, 3) and c[0, 0, 0].tolist() == [1, 1, 0] and c[0, 0, -1].tolist() == [0, 0, 0] and not c[:, 1].any()
    assert DN.half_steps(lo, np.zeros(1, int), 2)[0, 0].tolist() == lo[:, 0, 0].tolist()


def test_defaults():
    from tropical_cyclone_risk_amd import duration
    assert np.allclose(duration.DEFAULT_LEVELS, [17.49, 25.72, 32.92], atol=0.005)
    assert np.array_equal(duration.DEFAULT_LEVELS, np.array([34.0, 50.0, 64.0]) * 1852.0 / 3600.0)
    assert duration.DEFAULT_HOURS.tolist() == [1, 3, 6, 12, 24, 48]
    assert duration.hours_per_half_step(3600.0, 4) == 0.125


def test_argument_errors_before_any_device_work():
    from tropical_cyclone_risk_amd import duration
    rng = np.random.default_rng(0)
    lon, lat, v = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    env = [np.zeros((3, 5))] * 4
    base = dict(lon=lon, lat=lat, v=v, env=env, groups=np.zeros(3, np.int64), site_lon=np.array([280.0]), site_lat=np.array([20.0]),
                dt_s=DT)
    bad = [dict(levels=[20.0, 10.0]), dict(levels=[10.0, 10.0]),                      # not ascending
           dict(levels=[0.0, 10.0]), dict(levels=[-1.0]), dict(levels=[np.nan]), dict(levels=[10.0, np.inf]),    # <= 0, not finite
           dict(levels=np.arange(1.0, 10.0)), dict(levels=[]),                        # more than 8, none
           dict(levels=[10.0, 20.0, 30.0], thresholds=np.arange(1.0, 23.0)),          # 3 * 22 = 66 cells
           dict(levels=np.arange(1.0, 9.0), thresholds=np.arange(1.0, 9.0)),          # 8 * 9 = 72 cells
           dict(thresholds=[3.0, 1.0]), dict(thresholds=[0.0, 1.0]), dict(thresholds=[]), dict(thresholds=[1.0, np.inf]),
           dict(return_hours=[3]), dict(return_hours=[0, 0]), dict(return_hours='x'),
           # the footprint's own rules
           dict(r_out_km=0.0), dict(r_out_km=2000.5), dict(substeps=0), dict(substeps=65), dict(substeps=1.5), dict(ck_cd=2.0),
           dict(dt_s=0.0), dict(rmax_km=-5.0), dict(rmax_km=np.full((3, 4), 20.0)), dict(env=env[:3]), dict(v=v[:, :4]),
           dict(groups=np.zeros(2, np.int64)), dict(site_lat=np.array([np.nan])), dict(groups=np.array([0, 1, 2]), n_groups=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            duration.site_duration(**dict(base, **kw))
    # the limit itself passes the checks: 8 * 8 and 1 * 64 cells
    duration._check_levels(np.arange(1.0, 9.0), np.arange(1.0, 8.0), True)
    duration._check_levels([5.0], np.arange(1.0, 64.0), [0])


def test_cli_arguments(capsys):
    from tropical_cyclone_risk_amd import duration
    a = duration.parse_args(['x.nc', '--site', '1,2'])
    assert np.array_equal(a.levels, duration.DEFAULT_LEVELS) and np.array_equal(a.thresholds, duration.DEFAULT_HOURS)
    assert a.r_out_km == 500.0 and a.substeps == 1 and a.rmax_km is None and a.ck_cd is None and a.out == 'duration.npz'
    assert a.return_periods is None
    b = duration.parse_args(['x.nc', '--grid', '270:271:0.5,20:21:1', '--levels', '17.5,25.7,32.9', '--thresholds', '2:10:4',
                             '--r-out-km', '300', '--substeps', '4', '--return-periods', '10,50'])
    assert b.levels.tolist() == [17.5, 25.7, 32.9] and b.thresholds.tolist() == [2, 6, 10] and b.substeps == 4
    assert list(b.return_periods) == [10.0, 50.0]
    for argv in (['x.nc'], ['x.nc', '--site', '1,2', '--levels', '30,20'], ['x.nc', '--site', '1,2', '--levels', 'a,b'],
                 ['x.nc', '--site', '1,2', '--return-periods', '10', '--tail-exceedances', '5']):
        with pytest.raises(SystemExit):
            duration.parse_args(argv)
    assert 'not offered' in capsys.readouterr().err


def test_duration_symbols_exported(built_lib):
    from tropical_cyclone_risk_amd import _lib
    assert os.path.samefile(built_lib, _lib.LIB_PATH)
    L = _lib.lib()                                                      # (the package's own way in: one HIP runtime per process)
    for name in ('tcr_duration_dev', 'tcr_duration_host', 'tcr_duration_pairs'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name


# ------------------------------------------------------------------------------------------------------------------ GPU
def _tracks(seed):
    from tests.test_windfield import _groups, _stress_tracks
    rng = np.random.default_rng(seed)
    lon, lat, v, env = _stress_tracks(rng)
    groups, n_groups = _groups(rng, lon.shape[0])
    return rng, lon, lat, v, env, groups, n_groups


def _sites(rng, lon, lat, r_out):
    """251 sites: 30 on a centre, 16 planted at r_out from one, 125 in the core region of a storm, 40 out to 1.3 r_out, 20 of them
    again in the other longitude convention, 20 anywhere."""
    live = np.argwhere(np.isfinite(lon) & np.isfinite(lat))
    pick = live[rng.choice(len(live), 211, replace=False)]
    cl, ca = lon[pick[:, 0], pick[:, 1]], lat[pick[:, 0], pick[:, 1]]
    el, ea = WN.direct(cl[30:46], ca[30:46], np.full(16, r_out), rng.uniform(0, 6.3, 16))
    nl_, na_ = WN.direct(cl[46:171], ca[46:171], rng.uniform(5, min(120.0, r_out), 125), rng.uniform(0, 6.3, 125))
    fl_, fa_ = WN.direct(cl[171:], ca[171:], rng.uniform(5, 1.3 * r_out, 40), rng.uniform(0, 6.3, 40))
    slon = np.concatenate([cl[:30], el, nl_, fl_, nl_[:10] + 360.0, nl_[10:20] - 360.0, rng.uniform(-180, 360, 20)])
    slat = np.concatenate([ca[:30], ea, na_, fa_, na_[:20], rng.uniform(-50, 50, 20)])
    return slon, slat


# substeps, ck_cd, rm (None: Willoughby, a constant, 'plane'), r_out, levels, n_bin: n_level 3, 8, 1 and 8; 8 * 8 and 1 * 64 cells
CASES = [(1, 1.0, None, 500.0, (12.0, 18.0, 25.0), 6),
         (3, 0.5, 35.0, 300.0, (6.0, 9.0, 12.0, 15.0, 18.0, 21.0, 24.0, 28.0), 7),
         (6, 1.5, 'plane', 150.0, (15.0,), 63),
         (3, 1.0, 'plane', 800.0, (5.0, 8.0, 11.0, 14.0, 17.0, 20.0, 23.0, 26.0), 3)]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs of CASES[i] and the restatement on them (computed once, never changed)."""
    sub, c, rm, r_out, levels, n_bin = CASES[i]
    rng, lon, lat, v, env, groups, n_groups = _tracks(100 + i)
    if isinstance(rm, str):
        rm = rng.uniform(8.0, 90.0, lon.shape)
    slon, slat = _sites(rng, lon, lat, r_out)
    u = DN.unit_hours(DT, sub)
    thr = u * np.arange(1, n_bin + 1) * (2 if n_bin > 10 else 3 * sub)      # whole numbers of half-weights: ties are the normal case
    recs = WN.samples(lon, lat, v, env, DT, rmax_km=rm, substeps=sub)
    ref = DN.duration(recs, slon, slat, r_out, c, levels)
    for a in ref:
        a.setflags(write=False)
    kw = dict(levels=np.array(levels), thresholds=thr, rmax_km=rm, ck_cd=c, r_out_km=r_out, substeps=sub, n_groups=n_groups)
    return dict(tracks=(lon, lat, v, env, groups), sites=(slon, slat), kw=kw, u=u, ref=ref, n_groups=n_groups)


def _condition(ref):
    """What makes a case a test: (share of the possibly included cells without an ambiguous record, per level the exact cells with
    H > 0)."""
    lo, hi, n_amb, inc_any, _ = ref
    cells = np.broadcast_to(inc_any, lo.shape)
    exact = cells & (n_amb == 0)
    return exact.sum() / cells.sum(), [int((exact[l] & (lo[l] > 0)).sum()) for l in range(lo.shape[0])]


@pytest.mark.parametrize('i', range(len(CASES)))
def test_cases_are_decided_by_the_restatement(i):
    """Not a measurement: the cases are chosen so that nearly every cell has one allowed answer, and every level is reached."""
    share, reached = _condition(_case(i)['ref'])
    print('case %d: %.4f of the cells exact, exact cells with H > 0 per level %s' % (i, share, reached))
    assert share >= 0.95 and min(reached) >= 50
    assert _case(i)['sites'][0].size % 64 != 0


@functools.lru_cache(maxsize=None)
def _gpu(i):
    from tropical_cyclone_risk_amd import duration
    d = _case(i)
    lon, lat, v, env, groups = d['tracks']
    return duration.site_duration(lon, lat, v, env, groups, d['sites'][0], d['sites'][1], DT, return_hours=True, **d['kw'])


def _H(site_hours, u):
    """The integers behind a plane, which must reproduce it bit for bit; -1 where it is NaN."""
    nan = np.isnan(site_hours)
    H = np.where(nan, -1, np.rint(np.where(nan, 0.0, site_hours) / u)).astype(np.int64)
    assert LN.same_bits(site_hours, np.where(nan, np.nan, H.astype(np.float64) * u))
    return H


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(CASES)))
def test_gpu_matches_restatement(built_lib, i):
    d, r = _case(i), _gpu(i)
    lo, hi, n_amb, inc_any, inc_sure = d['ref']
    share, reached = _condition(d['ref'])
    assert share >= 0.95 and min(reached) >= 50
    sh = r['site_hours']
    assert sh.shape == lo.shape and r['hours_per_half_step'] == d['u']
    H = _H(sh, d['u'])
    nan = np.isnan(sh)
    assert (nan == nan[0]).all()                                        # NaN is the same at every level
    assert not (nan[0] & inc_sure).any() and not (~nan[0] & ~inc_any).any()
    ok = nan | ((lo <= H) & (H <= hi))
    assert ok.all(), [(int(l), int(a), int(s), int(H[l, a, s]), int(lo[l, a, s]), int(hi[l, a, s])) for l, a, s in np.argwhere(~ok)[:5]]
    exact = ~nan & (n_amb == 0)
    assert (H[exact] == lo[exact]).all()
    assert (np.diff(np.where(nan, 0, H), axis=0) <= 0).all()            # hours do not increase with the level
    assert np.isnan(sh[:, :, :5]).all()                                 # one-sample tracks


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(CASES)))
def test_gpu_counts_and_totals_from_own_planes(built_lib, i):
    d, r = _case(i), _gpu(i)
    groups, n_groups = d['tracks'][4], d['n_groups']
    sh = r['site_hours']
    H = _H(sh, d['u'])
    assert r['counts'].dtype == np.int32 and r['half_steps'].dtype == np.int64
    assert np.array_equal(r['counts'], DN.counts(sh, groups, n_groups, r['thresholds']))
    assert np.array_equal(r['half_steps'], DN.half_steps(np.maximum(H, 0), groups, n_groups))
    assert r['counts'].sum() > 100 and (np.diff(r['counts'], axis=3) <= 0).all() and (np.diff(r['counts'], axis=2) <= 0).all()
    for g in (1, 4):                                                    # the empty groups
        assert not r['counts'][:, g].any() and not r['half_steps'][:, g].any()


@pytest.mark.gpu
def test_gpu_agrees_with_the_footprint_exactly(built_lib):
    from tropical_cyclone_risk_amd import duration, windfield
    for i in (0, 1):                                                    # ck_cd 1 and not 1
        d, r = _case(i), _gpu(i)
        lon, lat, v, env, groups = d['tracks']
        slon, slat = d['sites']
        kw = {k: d['kw'][k] for k in ('rmax_km', 'ck_cd', 'r_out_km', 'substeps', 'n_groups')}
        m = windfield.site_wind(lon, lat, v, env, groups, slon, slat, DT, return_max=True, **kw)['site_max']
        sh = r['site_hours']
        for l, lev in enumerate(d['kw']['levels']):
            assert np.array_equal(np.isnan(sh[l]), np.isnan(m))
            with np.errstate(invalid='ignore'):
                assert np.array_equal(sh[l] > 0, m >= lev)
        # levels that are peaks themselves: >= and the footprint's own double, without a tolerance
        cand = np.argwhere(m > 1.0)
        src = cand[np.random.default_rng(i).choice(len(cand), 8, replace=False)]
        vals = m[src[:, 0], src[:, 1]]
        levels = np.unique(vals)
        r2 = duration.site_duration(lon, lat, v, env, groups, slon, slat, DT, levels=levels, thresholds=d['kw']['thresholds'][:5],
                                    return_hours=True, **kw)
        for (a, s), x in zip(src, vals):
            l = int(np.searchsorted(levels, x))
            assert levels[l] == x and r2['site_hours'][l, a, s] > 0
            assert l + 1 == levels.size or r2['site_hours'][l + 1, a, s] == 0.0
        with np.errstate(invalid='ignore'):
            for l, lev in enumerate(levels):
                assert np.array_equal(r2['site_hours'][l] > 0, m >= lev)


@pytest.mark.gpu
def test_gpu_bit_identical_across_runs_site_order_and_storm_order(built_lib):
    from tropical_cyclone_risk_amd import duration
    d, a = _case(3), _gpu(3)
    lon, lat, v, env, groups = d['tracks']
    slon, slat = d['sites']
    rng = np.random.default_rng(5)
    kw = dict(d['kw'], return_hours=True)

    def same(x, y, sites=slice(None), storms=slice(None)):
        assert np.array_equal(x['site_hours'].view(np.int64), y['site_hours'][:, sites][:, :, storms].view(np.int64))
        assert np.array_equal(x['counts'], y['counts'][sites]) and np.array_equal(x['half_steps'], y['half_steps'][sites])
    same(duration.site_duration(lon, lat, v, env, groups, slon, slat, DT, **kw), a)
    ps = rng.permutation(slon.size)
    same(duration.site_duration(lon, lat, v, env, groups, slon[ps], slat[ps], DT, **kw), a, sites=ps)
    pt = rng.permutation(lon.shape[0])                                  # storms shuffled within and across groups
    rm = kw['rmax_km'][pt]
    same(duration.site_duration(lon[pt], lat[pt], v[pt], [e[pt] for e in env], groups[pt], slon, slat, DT, **dict(kw, rmax_km=rm)), a,
         storms=pt)


@pytest.mark.gpu
def test_gpu_host_and_device_entry_points_agree(built_lib):
    import types
    import torch
    from tropical_cyclone_risk_amd import _lib, duration
    d, ref = _case(2), _gpu(2)
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
                r = duration.site_duration(t[0], t[1], t[2], t[3:7], groups, t[7], t[8], DT, engine=eng, return_hours=want,
                                           **dict(d['kw'], rmax_km=t[9]))
            side.synchronize()
            assert r['counts'].device == dev and r['half_steps'].device == dev
            assert np.array_equal(r['counts'].cpu().numpy(), ref['counts'])
            assert np.array_equal(r['half_steps'].cpu().numpy(), ref['half_steps'])
            if want is not False:
                assert LN.same_bits(r['site_hours'].cpu().numpy(), ref['site_hours'])
            else:
                assert 'site_hours' not in r
    finally:
        side.synchronize()
        _lib.lib().tcr_ctx_destroy(h)
    # planes for some of the levels only: the others are NaN, and nothing else moves
    d1, full = _case(1), _gpu(1)
    lon, lat, v, env, groups = d1['tracks']
    part = duration.site_duration(lon, lat, v, env, groups, d1['sites'][0], d1['sites'][1], DT, return_hours=[6, 2], **d1['kw'])
    for l in range(8):
        assert LN.same_bits(part['site_hours'][l], full['site_hours'][l]) if l in (2, 6) else np.isnan(part['site_hours'][l]).all()
    assert np.array_equal(part['counts'], full['counts']) and np.array_equal(part['half_steps'], full['half_steps'])
    # no storms at all
    e = duration.site_duration(lon[:0], lat[:0], v[:0], [x[:0] for x in env], groups[:0], d1['sites'][0], d1['sites'][1], DT,
                               return_hours=True, **dict(d1['kw'], n_groups=2))
    assert e['site_hours'].shape == (8, d1['sites'][0].size, 0) and e['counts'].shape == (d1['sites'][0].size, 2, 8, 7)
    assert not e['counts'].any() and not e['half_steps'].any()


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
        lev0, thr0 = np.array([0.5, 15.0, 25.0]), np.array([1.0, 3.0, 6.0])
        trk = _lib.WindTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=planes[0].ctypes.data, lat=planes[1].ctypes.data,
                              v=planes[2].ctypes.data, u250=planes[3].ctypes.data, v250=planes[4].ctypes.data,
                              u850=planes[5].ctypes.data, v850=planes[6].ctypes.data, rmax_km=None, n_group=2, group_off=off)

        def call(levels=lev0, thr=thr0, half=True, hours=None, no_array=False, **p):
            prm = _lib.WindParams(**dict(dict(dt_s=DT, ck_cd=1.0, r_out_km=500.0, rmax_const_km=0.0, substeps=2), **p))
            n_level, n_bin = len(levels), len(thr)
            counts = np.full((n_site, 2, n_level, n_bin), -7, np.int32)
            hs = np.full((n_site, 2, n_level), -7, np.int64)
            sh = np.full((max(n_level, 1), n_site, n_trk), -7.0)
            arr = (ctypes.c_void_p * max(n_level, 1))()
            for l in range(n_level) if hours is None else hours:
                arr[l] = sh[l].ctypes.data
            lv, th = np.asarray(levels, float), np.asarray(thr, float)
            rc = L.tcr_duration_host(h, ctypes.byref(trk), ctypes.byref(prm), n_site, slon.ctypes.data, slat.ctypes.data, n_level,
                                     lv.ctypes.data_as(_lib.DP), n_bin, th.ctypes.data_as(_lib.DP), counts.ctypes.data,
                                     hs.ctypes.data if half else None, None if no_array else arr)
            return rc, counts, hs, sh
        rc, counts, hs, sh = call()
        assert rc == 0 and counts.sum() > 0 and (counts >= 0).all() and (hs >= 0).all() and hs.sum() > 0
        u = DT / (7200.0 * 2)
        assert np.array_equal(hs, DN.half_steps(np.rint(sh / u).astype(np.int64), np.array([0, 0, 1]), 2))
        assert sh[0, 0, 0] == n_t - 1 and sh[0, 0, 2] == 3.0           # every record of the track blows at 0.5 m/s there
        pairs, wpairs = ctypes.c_int64(), ctypes.c_int64()
        assert L.tcr_duration_pairs(h, ctypes.byref(pairs)) == 0 and pairs.value > 0
        # outputs left out: the others are what they were, and nothing is written where nothing was asked for
        for kw in (dict(half=False), dict(hours=(1,)), dict(hours=()), dict(no_array=True), dict(half=False, no_array=True)):
            rc, c2, h2, s2 = call(**kw)
            assert rc == 0 and np.array_equal(c2, counts), kw
            assert np.array_equal(h2, hs) if kw.get('half', True) else (h2 == -7).all()
            for l in range(3):
                assert np.array_equal(s2[l], sh[l]) if (l in kw.get('hours', (0, 1, 2)) and not kw.get('no_array')) else (s2[l] == -7).all()
        # the footprint evaluates the same pairs
        wc = np.zeros((n_site, 2, 3), np.int32)
        prm = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=500.0, rmax_const_km=0.0, substeps=2)
        assert L.tcr_windfield_host(h, ctypes.byref(trk), ctypes.byref(prm), n_site, slon.ctypes.data, slat.ctypes.data, 3,
                                    lev0.ctypes.data_as(_lib.DP), wc.ctypes.data, None) == 0
        assert L.tcr_windfield_pairs(h, ctypes.byref(wpairs)) == 0 and wpairs.value == pairs.value
        bad = [dict(levels=[15.0, 5.0]), dict(levels=[0.0, 5.0]), dict(levels=[5.0, np.nan]), dict(levels=np.arange(1.0, 10.0), thr=[1.0]),
               dict(levels=[]), dict(thr=[3.0, 1.0]), dict(thr=[0.0, 1.0]), dict(thr=[-1.0]), dict(thr=[]),
               dict(levels=[1.0, 2.0, 3.0], thr=np.arange(1.0, 23.0)), dict(levels=np.arange(1.0, 9.0), thr=np.arange(1.0, 9.0), hours=()),
               dict(r_out_km=2001.0), dict(substeps=65), dict(ck_cd=2.0), dict(dt_s=0.0), dict(rmax_const_km=-1.0)]
        for kw in bad:
            assert call(**kw)[0] == -1, kw
            assert L.tcr_last_error(h).startswith(b'tcr_duration:'), (kw, L.tcr_last_error(h))
        assert call(levels=np.arange(1.0, 9.0), thr=np.arange(1.0, 8.0), hours=())[0] == 0      # 64 cells
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_cli_round_trip(built_lib, tmp_path, capsys):
    from tests.test_levels import _write_track_file
    from tropical_cyclone_risk_amd import analysis, duration, hazard, levels
    fn = _write_track_file(tmp_path, np.random.default_rng(5))
    sites = ['--site=-75.0,24.0', '--site', '286.5,25.5', '--site=-72.25,27.0', '--site', '10.0,50.0']
    opts = ['--levels', '12,18,26', '--thresholds', '3:30:9', '--substeps', '2']
    keys = {'counts', 'return_period', 'annual_hours', 'levels', 'thresholds', 'site_lon', 'site_lat', 'total_years', 'dt_s',
            'group_file', 'group_year', 'files'}
    out = str(tmp_path / 'duration.npz')
    assert duration.main([fn, '--out', out] + sites + opts) == 0
    plain = np.load(out)
    assert set(plain.files) == keys
    assert 'hours per year' in capsys.readouterr().out
    lon, lat, vmax, v, env, groups, gfile, gyear, dt = analysis.load_wind_planes([fn])
    api = duration.site_duration(lon, lat, v, env, groups, plain['site_lon'], plain['site_lat'], dt, levels=[12.0, 18.0, 26.0],
                                 thresholds=[3.0, 12.0, 21.0, 30.0], substeps=2, n_groups=3, return_hours=True)
    assert int(plain['total_years']) == 3 and float(plain['dt_s']) == dt and plain['levels'].tolist() == [12.0, 18.0, 26.0]
    assert plain['thresholds'].tolist() == [3.0, 12.0, 21.0, 30.0]
    assert np.array_equal(plain['counts'], api['counts']) and api['counts'].sum() > 0 and plain['counts'].shape == (4, 3, 3, 4)
    assert np.array_equal(plain['return_period'], hazard.return_periods(api['counts'], 3))
    assert np.array_equal(plain['annual_hours'], api['half_steps'].sum(1) * api['hours_per_half_step'] / 3)
    assert plain['annual_hours'].shape == (4, 3) and plain['annual_hours'][:3, 0].min() > 0 and not plain['annual_hours'][3].any()
    assert duration.main([fn, '--out', out, '--return-periods', '2,5'] + sites + opts) == 0
    z = np.load(out)
    assert set(z.files) == keys | {'return_level', 'return_periods', 'n_reach'}
    for name in keys:
        assert np.all((z[name] == plain[name]) | ((z[name] != z[name]) & (plain[name] != plain[name]))), name
    k, ok = levels.ranks_of_periods([2.0, 5.0], 3)
    assert z['return_level'].shape == (4, 3, 2) and np.array_equal(z['return_periods'], [2.0, 5.0])
    for l in range(3):
        want, n_reach = LN.row_select(api['site_hours'][l], k)
        want[:, ~ok] = np.nan
        assert LN.same_bits(z['return_level'][:, l], want) and np.array_equal(z['n_reach'], n_reach)
    assert not np.isnan(z['return_level'][:3, 0, 0]).any() and np.isnan(z['return_level'][3]).all()
