"""The permutation round trip of sitescan.site_scan, for its seven users (eight calls: the rainfall has two statistics).
Whatever order the caller's sites and storms are in, every returned array is, bit for bit, that of the same call on sites and
storms already in the order the front end chooses (storms of a group next to each other, sites in Z-order), mapped back to the
caller's order."""
import numpy as np
import pytest

N_T, N_GROUPS, DT = 5, 3, 3600.0
THR = np.array([20.0, 35.0, 50.0])
RTHR = {'total': np.array([1.0, 10.0, 30.0]), 'peak-rate': np.array([0.5, 3.0, 8.0])}      # mm, mm/h
LEVELS, HOURS = np.array([20.0, 35.0]), np.array([1.0, 2.0, 3.0])                           # m/s, hours (a track lasts 4)
WINDOWS_H = (1.0, 3.0)                  # hours: 1 and 3 samples of DT
# 49 storms: group sizes 33 / 0 / 16.  A chunk of the scan holds at least 16 storms, so the first group spans three chunks
# (16 + 16 + 1): the cross-chunk reductions and the per-chunk histograms' sums have more than one term
N_TRK = (0, 1, 17, 49)
N_SITE = (1, 64, 65)                    # one lane, a full tile, a second tile with one lane
# (5 - 1) 8 + 1 = 33 records: two culling segments, the second with one record and padding
SUBSTEPS = 8
NAMES = ['site_hazard', 'site_wind', 'portfolio_loss', 'site_rain-total', 'site_rain-peak-rate', 'site_compound', 'site_duration',
         'site_accumulation']
PAIR_PLANES = ('site_max', 'site_total', 'site_peak_rate', 'site_wind', 'site_rain')        # [n_site][n_trk]


def _storms(rng, n):
    """n storms of N_T samples in the box 278..284 E, 24..28 N, moving about 0.2 degrees an hour; every fourth ends two samples
    early (NaN tail); groups unsorted over N_GROUPS = 3 with the middle group empty: every third storm before the 49th is in the
    last group."""
    step = rng.normal(0.0, 0.2, (2, n, N_T))
    step[:, :, 0] = 0.0
    P = dict(lon=rng.uniform(278, 284, (n, 1)) + np.cumsum(step[0], axis=1), lat=rng.uniform(24, 28, (n, 1)) + np.cumsum(step[1], axis=1),
             vmax=rng.uniform(25, 70, (n, N_T)), v=rng.uniform(20, 65, (n, N_T)))
    for k in ('u250', 'v250', 'u850', 'v850'):
        P[k] = rng.normal(0.0, 8.0, (n, N_T))
    for a in P.values():
        a[1::4, N_T - 2:] = np.nan
    return P, np.where((np.arange(n) % 3 == 0) & (np.arange(n) < 48), 2, 0).astype(np.int64)


def _sites(rng, n):
    """n sites in the storms' box in random order, half of them in the -180..180 convention; value (one site with nothing
    exposed) and a v_half of their own."""
    lon, lat = rng.uniform(278, 284, n), rng.uniform(24, 28, n)
    lon = np.where(rng.random(n) < 0.5, lon - 360.0, lon)
    value = rng.lognormal(13.0, 1.5, n)
    value[n // 2] = 0.0
    return lon, lat, value, rng.uniform(60.0, 80.0, n)


def _run(name, P, groups, slon, slat, value, v_half, substeps=1):
    from tropical_cyclone_risk_amd import accumulation, compound, duration, hazard, loss, rainfall, windfield
    if name == 'site_hazard':
        return hazard.site_hazard(P['lon'], P['lat'], P['vmax'], groups, slon, slat, radius_km=300.0, thresholds=THR,
                                  return_max=True, n_groups=N_GROUPS)
    if name.startswith('site_rain'):
        stat = name[len('site_rain-'):]
        return rainfall.site_rain(P['lon'], P['lat'], P['vmax'], groups, slon, slat, DT, stat=stat, substeps=substeps,
                                  thresholds=RTHR[stat], return_values=True, n_groups=N_GROUPS)
    if name == 'site_accumulation':
        return accumulation.site_accumulation(P['lon'], P['lat'], P['vmax'], groups, slon, slat, DT, windows_h=WINDOWS_H,
                                              thresholds=RTHR['total'], substeps=substeps, return_values=True, n_groups=N_GROUPS)
    env = [P[k] for k in ('u250', 'v250', 'u850', 'v850')]
    if name == 'site_wind':
        return windfield.site_wind(P['lon'], P['lat'], P['v'], env, groups, slon, slat, DT, substeps=substeps, thresholds=THR,
                                   return_max=True, n_groups=N_GROUPS)
    if name == 'site_compound':
        return compound.site_compound(P['lon'], P['lat'], P['v'], P['vmax'], env, groups, slon, slat, DT, THR, RTHR['total'],
                                      substeps=substeps, return_values=True, n_groups=N_GROUPS)
    if name == 'site_duration':
        return duration.site_duration(P['lon'], P['lat'], P['v'], env, groups, slon, slat, DT, levels=LEVELS, thresholds=HOURS,
                                      substeps=substeps, return_hours=True, n_groups=N_GROUPS)
    return loss.portfolio_loss(P['lon'], P['lat'], P['v'], env, groups, slon, slat, value, DT, v_half=v_half, substeps=substeps,
                               thresholds=THR, n_groups=N_GROUPS)


def _echo(name, substeps):
    """what a result repeats of the call: the same whatever the order"""
    from tropical_cyclone_risk_amd import duration
    if name.startswith('site_rain'):
        return dict(thresholds=RTHR[name[len('site_rain-'):]])
    if name == 'site_compound':
        return dict(wind_thresholds=THR, rain_thresholds=RTHR['total'])
    if name == 'site_duration':
        return dict(thresholds=HOURS, levels=LEVELS, hours_per_half_step=duration.hours_per_half_step(DT, substeps))
    if name == 'site_accumulation':
        return dict(thresholds=RTHR['total'], windows_h=np.array(WINDOWS_H), window_samples=np.array([1, 3], dtype=np.int32))
    return dict(thresholds=THR)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()     # (NaNs by their bit pattern)


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_gpu_results_come_back_in_the_callers_order(built_lib, name):
    import torch
    from tropical_cyclone_risk_amd import sitescan
    rng = np.random.default_rng(11)
    Pall, gall = _storms(rng, max(N_TRK))
    assert np.array_equal(np.bincount(gall, minlength=N_GROUPS), [33, 0, 16])
    dev = torch.device('cuda', 0)
    Tall = {k: torch.as_tensor(a, device=dev) for k, a in Pall.items()}
    side = torch.cuda.Stream(dev)
    for n_site in N_SITE:
        slon, slat, value, v_half = _sites(rng, n_site)
        site_order = sitescan.spatial_order(slon, slat, np)
        assert n_site == 1 or not np.array_equal(site_order, np.arange(n_site))
        cases = [(n_trk, 1) for n_trk in N_TRK]
        if name != 'site_hazard' and n_site == max(N_SITE):
            cases.append((max(N_TRK), SUBSTEPS))
        for n_trk, substeps in cases:
            # (a caller without storms holds empty slices of its planes, on the device as well)
            P, groups = {k: a[:n_trk] for k, a in Pall.items()}, gall[:n_trk]
            order = np.argsort(groups, kind='stable')
            assert n_trk < 2 or not np.array_equal(order, np.arange(n_trk))
            got = _run(name, P, groups, slon, slat, value, v_half, substeps)

            # the same call in the front end's order, mapped back
            ref = _run(name, {k: a[order] for k, a in P.items()}, groups[order], slon[site_order], slat[site_order],
                       value[site_order], v_half[site_order], substeps)
            echo = _echo(name, substeps)
            want = dict(echo)
            for k, a in ref.items():
                if k in ('counts', 'site_loss', 'half_steps'):          # along the sites (a ('site_group', k) output too)
                    want[k] = np.empty_like(a)
                    want[k][site_order] = a
                elif k in PAIR_PLANES:
                    want[k] = np.empty_like(a)
                    want[k][np.ix_(site_order, order)] = a
                elif k in ('site_hours', 'site_window'):                # a 'pair' plane per level or window
                    want[k] = np.empty_like(a)
                    want[k][np.ix_(np.arange(a.shape[0]), site_order, order)] = a
                elif k == 'event_loss':
                    want[k] = np.empty_like(a)
                    want[k][order] = a
                elif k in ('year_agg', 'year_max'):
                    want[k] = a
            assert set(got) == set(ref) == set(want)
            shapes = dict(counts=(n_site, N_GROUPS, THR.size), site_max=(n_site, n_trk), event_loss=(n_trk,), year_agg=(N_GROUPS,),
                          year_max=(N_GROUPS,), site_loss=(n_site,), thresholds=THR.shape, site_total=(n_site, n_trk),
                          site_peak_rate=(n_site, n_trk), site_wind=(n_site, n_trk), site_rain=(n_site, n_trk),
                          wind_thresholds=THR.shape, rain_thresholds=THR.shape, levels=LEVELS.shape, hours_per_half_step=(),
                          half_steps=(n_site, N_GROUPS, LEVELS.size), site_hours=(LEVELS.size, n_site, n_trk),
                          windows_h=(len(WINDOWS_H),), window_samples=(len(WINDOWS_H),), site_window=(len(WINDOWS_H), n_site, n_trk))
            if name == 'site_compound':
                shapes['counts'] = (n_site, N_GROUPS, THR.size + 1, THR.size + 1)
            elif name == 'site_duration':
                shapes['counts'] = (n_site, N_GROUPS, LEVELS.size, HOURS.size)
            elif name == 'site_accumulation':
                shapes['counts'] = (n_site, N_GROUPS, len(WINDOWS_H), THR.size)
            for k in want:
                assert np.shape(got[k]) == shapes[k] and _same_bits(got[k], want[k]), (k, n_site, n_trk, substeps)

            # torch tensors on a side stream, with a context of the call's own
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                r = _run(name, {k: a[:n_trk] for k, a in Tall.items()}, groups, *(torch.as_tensor(a, device=dev) for a in
                                                                                  (slon, slat, value, v_half)), substeps)
            side.synchronize()
            assert set(r) == set(got)
            for k in got:
                if k not in echo:
                    assert r[k].device == dev, k
                assert _same_bits(r[k].cpu().numpy() if k not in echo else r[k], got[k]), (k, n_site, n_trk, substeps)

            if n_trk == 0:
                assert not got['counts'].any()
                for k in ('event_loss', 'year_agg', 'year_max', 'site_loss', 'half_steps'):
                    assert k not in got or not got[k].any(), k
            elif n_trk == max(N_TRK) and n_site >= 64:              # (the cases are not empty)
                assert got['counts'][:, 0].sum() > 0 and got['counts'][:, 2].sum() > 0 and not got['counts'][:, 1].any()
                if name == 'portfolio_loss':
                    assert (got['event_loss'] > 0).sum() > 1 and got['year_agg'][1] == 0.0 and (got['site_loss'] > 0).sum() > 1
                elif name == 'site_compound':
                    assert np.isfinite(got['site_wind']).sum() > n_site and np.isfinite(got['site_rain']).sum() > n_site
                    assert got['counts'][:, :, 1:, 1:].sum() > 0                # some storm passes a threshold of each list
                elif name == 'site_duration':
                    assert (got['half_steps'][:, 0] > 0).sum() > 1 and not got['half_steps'][:, 1].any()
                    assert np.isfinite(got['site_hours']).sum() > n_site and (got['site_hours'] > 0).sum() > n_site
                elif name == 'site_accumulation':
                    assert np.isfinite(got['site_window']).sum() > n_site
                else:
                    plane = [k for k in PAIR_PLANES if k in got]
                    assert len(plane) == 1 and np.isfinite(got[plane[0]]).sum() > n_site


@pytest.mark.parametrize('arg_name,row_name', [('return_hours', 'level'), ('return_values', 'window')])
def test_wanted_rows(arg_name, row_name):
    """The rows whose planes a stacked analysis returns: duration's return_hours and accumulation's return_values."""
    from tropical_cyclone_risk_amd.sitescan import wanted_rows
    rows = lambda v, n=4: wanted_rows(v, n, arg_name, row_name)                             # noqa: E731
    assert rows(True) == [0, 1, 2, 3] and rows(True, 1) == [0]
    assert rows(False) == [] and rows(None) == [] and rows([]) == [] and rows(()) == []
    assert rows([2, 0]) == [0, 2] and rows((3, 1, 2)) == [1, 2, 3] and rows([1.0]) == [1]
    got = rows(np.array([3, 0], dtype=np.int64))
    assert got == [0, 3] and all(type(i) is int for i in got)
    not_a_list = '%s must be True, False or a list of distinct %s indices' % (arg_name, row_name)
    for bad in ([1, 1], (0, 2, 0), np.array([2, 2]), [True], [0, False], [0.5], [1, 'a'], ['1'], 3, 'all', [None], [[0]]):
        with pytest.raises(ValueError) as e:
            rows(bad)
        assert str(e.value) == not_a_list, bad
    for bad in ([4], [-1], (0, 7), np.array([1, 4])):
        with pytest.raises(ValueError) as e:
            rows(bad)
        assert str(e.value) == '%s names a %s that does not exist' % (arg_name, row_name), bad
    assert rows([3]) == [3] and rows([0], 1) == [0]


# ------------------------------------------------------------------------------------------- the checks the analyses share
DT_TEXT = 'dt_s must be finite and > 0'
R_OUT_TEXT = 'r_out_km must be in (0, 2000]'
SUBSTEPS_TEXT = 'substeps must be an integer in [1, 64]'
N_GROUPS_TEXT = 'n_groups must be >= 1'
BOUNDED_TEXT = 'thresholds must be 1 to 64 finite, strictly ascending values'
ASCENDING_TEXT = 'thresholds must be finite and strictly ascending'
POSITIVE_TEXT = 'thresholds must be finite, > 0 and strictly ascending'
LONG = np.arange(1.0, 66.0)             # 65 thresholds


def _public_calls():
    """name -> (the public function on three storms and one site, given keywords; the name of its r_out_km; the names of its
    threshold lists; the text of a bad list; the text of a list of 65)."""
    from tropical_cyclone_risk_amd import accumulation, compound, directional, duration, hazard, loss, rainfall, windfield
    rng = np.random.default_rng(0)
    lon, lat, v = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    env, g, slon, slat = [np.zeros((3, 5))] * 4, np.zeros(3, np.int64), np.array([280.0]), np.array([20.0])

    def wind(fn, *more):
        return lambda dt_s=DT, **kw: fn(lon, lat, v, env, g, slon, slat, *more, dt_s, **kw)

    def rain(fn):
        return lambda dt_s=DT, **kw: fn(lon, lat, v, g, slon, slat, dt_s, **kw)
    return {
        'site_hazard': (lambda dt_s=None, **kw: hazard.site_hazard(lon, lat, v, g, slon, slat, **kw), None, (), None, None),
        'site_wind': (wind(windfield.site_wind), 'r_out_km', ('thresholds',), BOUNDED_TEXT, BOUNDED_TEXT),
        'portfolio_loss': (wind(loss.portfolio_loss, np.ones(1)), 'r_out_km', ('thresholds',), BOUNDED_TEXT, BOUNDED_TEXT),
        'site_rain': (rain(rainfall.site_rain), 'r_out_km', ('thresholds',), BOUNDED_TEXT, BOUNDED_TEXT),
        'site_compound': (lambda dt_s=DT, wind_thresholds=THR, rain_thresholds=THR, **kw: compound.site_compound(
            lon, lat, v, v, env, g, slon, slat, dt_s, wind_thresholds, rain_thresholds, **kw), 'wind_r_out_km',
            ('wind_thresholds', 'rain_thresholds'), BOUNDED_TEXT, BOUNDED_TEXT),
        'site_duration': (wind(duration.site_duration), 'r_out_km', ('thresholds',), POSITIVE_TEXT, 'n_level * (n_bin + 1) must be <= 64'),
        'site_accumulation': (rain(accumulation.site_accumulation), 'r_out_km', ('thresholds',), ASCENDING_TEXT,
                              'n_window * (n_bin + 1) must be <= 64'),
        'site_directional_wind': (wind(directional.site_directional_wind), 'r_out_km', ('thresholds',), ASCENDING_TEXT,
                                  'n_sector * (n_bin + 1) must be <= 64')}


@pytest.fixture
def nothing_loaded(monkeypatch):
    """The library as in a process that has not loaded it; whoever loads it leaves it in _lib._lib."""
    from tropical_cyclone_risk_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    yield
    assert _lib._lib is None


def _raises(call, text, **kw):
    with pytest.raises(ValueError) as e:
        call(**kw)
    assert str(e.value) == text, kw


@pytest.mark.parametrize('name', ['site_hazard', 'site_wind', 'portfolio_loss', 'site_rain', 'site_compound', 'site_duration',
                                  'site_accumulation', 'site_directional_wind'])
def test_shared_checks_keep_their_texts(name, nothing_loaded):
    """One bad value per rule of the checks the analyses share, at every public function that has the rule: the ValueError's
    text is what it was when each module wrote the check out, and the library is not loaded."""
    call, r_out, thr_names, bad_text, long_text = _public_calls()[name]
    if name == 'site_hazard':           # none of the rules: the library checks its radius and thresholds, site_scan its groups
        _raises(call, 'a group index is >= n_groups', n_groups=0)
        return
    for dt in (0.0, np.nan):
        _raises(call, DT_TEXT, dt_s=dt)
    for r in (0.0, 2000.1):
        _raises(call, R_OUT_TEXT, **{r_out: r})
    if name == 'site_compound':
        _raises(call, R_OUT_TEXT, rain_r_out_km=2000.1)
    for s in (0, 65, 1.5, True):
        _raises(call, SUBSTEPS_TEXT, substeps=s)
    _raises(call, N_GROUPS_TEXT, n_groups=0)
    for thr_name in thr_names:
        for bad in ([], [10.0, np.nan], [30.0, 20.0]):
            _raises(call, bad_text, **{thr_name: bad})
        _raises(call, long_text, **{thr_name: LONG})


def test_shared_checks_keep_their_order(nothing_loaded):
    """A call that breaks two rules gets the ValueError it always got."""
    calls = {k: c[0] for k, c in _public_calls().items()}
    _raises(calls['site_wind'], DT_TEXT, dt_s=0.0, substeps=0)
    _raises(calls['site_wind'], 'ck_cd must be in (0, 2)', ck_cd=2.0, r_out_km=0.0)
    _raises(calls['site_wind'], 'rmax_km must be finite and > 0', rmax_km=-5.0, n_groups=0)
    _raises(calls['site_rain'], R_OUT_TEXT, r_out_km=0.0, thresholds=[])
    _raises(calls['site_rain'], "stat must be 'total' or 'peak-rate'", stat='mean', dt_s=0.0)
    _raises(calls['portfolio_loss'], SUBSTEPS_TEXT, substeps=0, n_groups=0)
    _raises(calls['portfolio_loss'], N_GROUPS_TEXT, n_groups=0, v_thresh=-1.0)
    _raises(calls['site_compound'], BOUNDED_TEXT, wind_thresholds=[], rain_r_out_km=0.0)
    _raises(calls['site_compound'], R_OUT_TEXT, wind_r_out_km=0.0, rain_thresholds=[])
    _raises(calls['site_compound'], N_GROUPS_TEXT, n_groups=0, stat='mean')
    _raises(calls['site_duration'], 'levels must be finite, > 0 and strictly ascending', levels=[20.0, 10.0], dt_s=0.0)
    _raises(calls['site_duration'], 'return_hours names a level that does not exist', return_hours=[3], dt_s=0.0)
    _raises(calls['site_directional_wind'], ASCENDING_TEXT, thresholds=[10.0, np.nan], r_out_km=0.0)
    _raises(calls['site_directional_wind'], 'return_max names a sector that does not exist', return_max=[8], substeps=0)
    _raises(calls['site_accumulation'], DT_TEXT, dt_s=0.0, windows_h=[3.0, 1.0])
    _raises(calls['site_accumulation'], 'give 1 to 8 windows', windows_h=[], r_out_km=0.0)
    _raises(calls['site_accumulation'], 'return_values names a window that does not exist', windows_h=[1.0], return_values=[1],
            substeps=0)
    # the rainfall knows its default thresholds by identity, and refuses them for the other statistic
    _raises(calls['site_rain'], "stat='peak-rate' needs explicit thresholds (mm/h): the defaults are storm totals in mm",
            stat='peak-rate')
    _raises(calls['site_rain'], N_GROUPS_TEXT, stat='peak-rate', thresholds=[1.0, 2.0], n_groups=0)
    # a dt_s that is no number: the accumulation's own text, the conversion's error everywhere else
    _raises(calls['site_accumulation'], DT_TEXT, dt_s=None)
    _raises(calls['site_accumulation'], DT_TEXT, dt_s='an hour')
    with pytest.raises(TypeError):
        calls['site_wind'](dt_s=None)
    with pytest.raises(TypeError):
        calls['site_rain'](dt_s=None)


# ---------------------------------------------------------------------------------------------------- the command lines
D_THR = [10.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 45.0, 50.0, 55.0, 60.0, 65.0, 70.0, 75.0, 80.0]
D_RAIN = [25.0, 50.0, 75.0, 100.0, 150.0, 200.0, 250.0, 300.0, 400.0, 500.0]
D_SITES = dict(site=[(1.0, 2.0)], sites=None, grid=None, tracks=['t.nc'], device=0)
D_PERIODS = dict(return_periods=None, tail_exceedances=None)
D_EVENTS = dict(events_out=None, events_min=None)
D_FOOTPRINT = dict(rmax_km=None, ck_cd=None, r_out_km=500.0, substeps=1)
PARSED = {
    'hazard': dict(D_SITES, **D_PERIODS, **D_EVENTS, out='hazard.npz', radius_km=100.0, thresholds=D_THR),
    'windfield': dict(D_SITES, **D_PERIODS, **D_EVENTS, **D_FOOTPRINT, out='wind.npz', thresholds=D_THR),
    'rainfall': dict(D_SITES, **D_PERIODS, **D_EVENTS, out='rain.npz', r_out_km=500.0, substeps=1, stat='total', thresholds=D_RAIN),
    'loss': dict(D_FOOTPRINT, tracks=['t.nc'], device=0, exposure='e.csv', out='loss.npz', return_periods=[10.0, 25.0, 50.0, 100.0, 250.0],
                 v_half=74.7, v_thresh=25.7),
    'compound': dict(D_SITES, **D_FOOTPRINT, out='compound.npz', wind_r_out_km=500.0, rain_r_out_km=500.0, stat='total',
                     wind_thresholds=[20.0, 30.0, 40.0, 50.0, 60.0, 70.0],
                     rain_thresholds=[50.0, 100.0, 150.0, 200.0, 250.0, 300.0, 350.0, 400.0]),
    'duration': dict(D_SITES, **D_PERIODS, **D_FOOTPRINT, out='duration.npz', thresholds=[1.0, 3.0, 6.0, 12.0, 24.0, 48.0],
                     levels=[34.0 * 1852.0 / 3600.0, 50.0 * 1852.0 / 3600.0, 64.0 * 1852.0 / 3600.0]),
    'accumulation': dict(D_SITES, **D_PERIODS, out='accumulation.npz', r_out_km=500.0, substeps=1, thresholds=D_RAIN,
                         windows=[6.0, 12.0, 24.0, 48.0, 72.0]),
    'directional': dict(D_SITES, **D_PERIODS, **D_FOOTPRINT, out='directional.npz', sectors=8, sector0_deg=0.0,
                        thresholds=[10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0])}
PARSED['compound'].pop('r_out_km')
NO_TAIL = {'duration': '--tail-exceedances is not offered for durations: they are quantised in half sub-steps, which a Pareto fit to '
                       'the excesses does not describe',
           'directional': "--tail-exceedances is not offered for directional wind: a sector's peaks have a point mass at 0 (storms "
                          'that reached the site with no wind from that sector), which a Pareto fit to the excesses does not describe',
           'accumulation': '--tail-exceedances is not offered for accumulation windows yet'}


def _exits_2(mod, argv, capsys, text):
    with pytest.raises(SystemExit) as e:
        mod.parse_args(argv)
    assert e.value.code == 2
    assert capsys.readouterr().err.endswith('python -m %s: error: %s\n' % (mod.__name__, text)), argv


@pytest.mark.parametrize('name', sorted(PARSED))
def test_parsers_keep_their_options_and_refusals(name, capsys):
    import importlib
    mod = importlib.import_module('tropical_cyclone_risk_amd.' + name)
    argv = ['t.nc', '--exposure', 'e.csv'] if name == 'loss' else ['t.nc', '--site=1,2']
    got = {k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in vars(mod.parse_args(argv)).items()}
    assert got == PARSED[name]
    if name == 'loss':                  # (an exposure file in place of sites)
        _exits_2(mod, ['t.nc'], capsys, 'the following arguments are required: --exposure')
        return
    _exits_2(mod, ['t.nc'], capsys, 'give sites with --site, --sites or --grid')
    if name in NO_TAIL:
        _exits_2(mod, argv + ['--return-periods', '10', '--tail-exceedances', '5'], capsys, NO_TAIL[name])
        _exits_2(mod, ['t.nc', '--tail-exceedances', '5'], capsys, NO_TAIL[name])           # (before the sites are missed)
    elif 'tail_exceedances' in PARSED[name]:
        _exits_2(mod, argv + ['--tail-exceedances', '5'], capsys, '--tail-exceedances needs --return-periods')
        _exits_2(mod, ['t.nc', '--tail-exceedances', '5'], capsys, '--tail-exceedances needs --return-periods')
        assert mod.parse_args(argv + ['--return-periods', '10', '--tail-exceedances', '5']).tail_exceedances == 5
    if 'events_out' in PARSED[name]:
        _exits_2(mod, argv + ['--events-out', 'e.npz'], capsys, '--events-out needs --events-min')
        _exits_2(mod, argv + ['--events-min', '20'], capsys, '--events-min needs --events-out')
        _exits_2(mod, ['t.nc', '--events-min', '20'], capsys, '--events-min needs --events-out')


def test_site_rows_are_printed_as_before(capsys):
    """print_site_rows and print_site_tables against the loops every command line wrote out before them."""
    from tropical_cyclone_risk_amd import analysis
    slon, slat = np.array([-80.1918, 286.5]), np.array([25.7617, 25.5])
    rows = np.array([[1.5, 20.0, np.inf], [3.0, 1000.0, 0.125]])
    analysis.print_site_rows('return period (years) by threshold (m/s): ' + ' '.join('%6g' % t for t in THR), slon, slat, rows, '%6.3g')
    want = ['return period (years) by threshold (m/s): ' + ' '.join('%6g' % t for t in THR)]
    want += ['  site (%.4f, %.4f): ' % (slon[i], slat[i]) + ' '.join('%6.3g' % v for v in rows[i]) for i in range(2)]
    assert want[1:] == ['  site (-80.1918, 25.7617):    1.5     20    inf', '  site (286.5000, 25.5000):      3  1e+03  0.125']
    assert capsys.readouterr().out == '\n'.join(want) + '\n'
    analysis.print_return_periods(THR, slon, slat, rows)
    assert capsys.readouterr().out == '\n'.join(want) + '\n'
    analysis.print_return_periods(THR, np.zeros(11), np.zeros(11), np.ones((11, 3)))        # more than 10 sites: nothing
    assert capsys.readouterr().out == ''
    analysis.print_site_rows(None, slon, slat, ['none', 'worst sector 2: 30 m/s every 4 years'])
    assert capsys.readouterr().out == ('  site (-80.1918, 25.7617): none\n'
                                       '  site (286.5000, 25.5000): worst sector 2: 30 m/s every 4 years\n')
    joint = np.stack([rows, 2.0 * rows])                                                   # [site][wind threshold][rain threshold]
    analysis.print_site_tables('joint', slon, slat, ['%6g: ' % u for u in (20.0, 35.0)], joint, '%6.3g')
    want = ['joint']
    for i in range(2):
        want.append('  site (%.4f, %.4f)' % (slon[i], slat[i]))
        for a, u in enumerate((20.0, 35.0)):
            want.append('    %6g: ' % u + ' '.join('%6.3g' % x for x in joint[i, a]))
    assert capsys.readouterr().out == '\n'.join(want) + '\n'


# -------------------------------------------------------------------------------------------------------- a bound scan
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['duration', 'directional', 'accumulation'])
def test_gpu_bound_scan_is_reusable(built_lib, name):
    """One binding, four calls: on all 70 sites (two tiles: 64 + 6), on each tile, and on all sites with both rows' planes.  The
    tiles put together are the whole call, and the last call is the public function's, bit for bit: what
    sitescan.stacked_return_levels relies on when it calls one bound scan per row and site block."""
    from tropical_cyclone_risk_amd import accumulation, directional, duration
    rng = np.random.default_rng(23)
    n, n_t = 12, 20
    step = rng.normal(0.0, 0.2, (2, n, n_t))
    step[:, :, 0] = 0.0
    lon, lat = rng.uniform(278, 284, (n, 1)) + np.cumsum(step[0], axis=1), rng.uniform(24, 28, (n, 1)) + np.cumsum(step[1], axis=1)
    vmax, v = rng.uniform(25, 70, (n, n_t)), rng.uniform(20, 65, (n, n_t))
    env = [rng.normal(0.0, 8.0, (n, n_t)) for _ in range(4)]
    for a in [lon, lat, vmax, v] + env:
        a[1::4, n_t - 3:] = np.nan
    groups = (np.arange(n) % 3 == 0).astype(np.int64)                   # 8 + 4 storms, not sorted
    slon, slat = rng.uniform(278, 284, 70), rng.uniform(24, 28, 70)
    if name == 'duration':
        tracks, key = (lon, lat, v, env), 'site_hours'
        scan = duration._bind(groups, DT, LEVELS, HOURS, None, None, 500.0, 2, 2)
        public = duration.site_duration(lon, lat, v, env, groups, slon, slat, DT, levels=LEVELS, thresholds=HOURS, substeps=2,
                                        return_hours=True, n_groups=2)
    elif name == 'directional':
        tracks, key = (lon, lat, v, env), 'site_dir_max'
        scan = directional._bind(groups, DT, 2, 0.0, THR, None, None, 500.0, 2, 2)
        public = directional.site_directional_wind(lon, lat, v, env, groups, slon, slat, DT, n_sector=2, thresholds=THR, substeps=2,
                                                   return_max=True, n_groups=2)
    else:
        tracks, key = (lon, lat, vmax), 'site_window'
        scan = accumulation._bind(groups, DT, WINDOWS_H, RTHR['total'], substeps=2, n_groups=2)
        public = accumulation.site_accumulation(lon, lat, vmax, groups, slon, slat, DT, windows_h=WINDOWS_H, thresholds=RTHR['total'],
                                                substeps=2, return_values=True, n_groups=2)
    whole, _ = scan(tracks, slon, slat, want=[1])
    tiles = [scan(tracks, slon[i:j], slat[i:j], want=[1])[0] for i, j in ((0, 64), (64, 70))]
    both, _ = scan(tracks, slon, slat, want=[0, 1])
    assert whole['counts'].shape == (70, 2, 2, 3) and whole['counts'].dtype == np.int32 and whole['counts'].sum() > 0
    assert sorted(whole['planes']) == [1] and whole['planes'][1].shape == (70, n) and np.isfinite(whole['planes'][1]).sum() > 70
    for k in ('counts', 'half_steps'):
        if k in whole:
            assert _same_bits(np.concatenate([t[k] for t in tiles]), whole[k]), k
    assert all(sorted(t['planes']) == [1] for t in tiles)
    assert _same_bits(np.concatenate([t['planes'][1] for t in tiles]), whole['planes'][1])
    assert sorted(both['planes']) == [0, 1] and _same_bits(both['planes'][1], whole['planes'][1])
    assert _same_bits(both['counts'], whole['counts']) and _same_bits(both['counts'], public['counts'])
    assert public[key].shape == (2, 70, n) and _same_bits(np.stack([both['planes'][0], both['planes'][1]]), public[key])
    assert set(both) - {'planes'} == set(public) - {key}
