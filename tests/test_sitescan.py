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
