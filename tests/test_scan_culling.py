"""The two claims every user of the site scan inherits from csrc/tcr_sitescan.h, held by tests of their own:

  "culling changes which pairs are evaluated, never a result"    the unculled twin: every analysis on one site set in two site
                                                                  orders, the front end's Morton order (culling active) and a
                                                                  spoiled order in which hz_far can skip nothing, bit for bit;
  "a skipped pair is always farther than R"                      the hazard (a pair's value is the sample's vmax: the result is
                                                                  decided by inclusion alone) at geometric edges and at radii
                                                                  of 1 to 5000 km, against the haversine in long double.

The spoiled order.  The first site of every tile of 64 is the tile cap's centre.  There it is an anchor: the exact antipode
(lon + 180, -lat) of the tile's second site.  The cap's radius rt is then (pi - gap) + r_ang + 2 kHzPad, where gap is the rounding
of the half-angle form at an antipodal pair; the tests assert gap < 1e-6 rad with a transcription of hz_a and hz_angle, far below
r_ang of any radius >= 1 km (1.6e-4 rad), so ``c.r + rt >= kPi`` holds for every storm and segment cap and every record meets
every site.  The anchors are ordinary sites of the set in both orders; the only difference between two runs is the permutation,
chosen by patching sitescan.spatial_order, which site_scan looks up at call time.

The edge layout (tests/scan_geometry_numpy.py) has, in the spoiled order, five tiles without an anchor: one of sites all over the
globe, whose cap is large but short of pi, and for every radius a compact "rim" tile whose cap reaches the stationary storm (a cap of
radius 0) by the R in its radius alone: a cap that loses its R, or part of it, loses the pair, and the reference notices.

With -s the tests print the pairs evaluated in both orders (profiles/scan_culling_census.txt)."""
import ctypes
import functools
import types

import numpy as np
import pytest

from tests import hazard_numpy as HN
from tests import loss_numpy as LN
from tests import scan_geometry_numpy as G

DT = 3600.0
U = LN.U
THR = np.array([20.0, 35.0, 50.0])
RTHR = np.array([1.0, 10.0, 30.0])              # mm
PTHR = np.array([0.5, 3.0, 8.0])                # mm/h
MAX_GAP = 1e-6                                  # rad: pi - angle(anchor, partner), far below 1 km / 6378 km = 1.57e-4
RE_HAZARD, RE_OTHERS = 6378.0, 6378.1           # km: kHzRe and kWfEarthR / 1000
CLUSTERS = 26                                   # compact patches of 63 sites in the twin's site set: 32 tiles in all
needs_long_double = pytest.mark.skipif(not G.LD_IS_WIDER, reason='np.longdouble is not wider than fp64 on this host: no reference')


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()     # (NaNs by their bit pattern)


@pytest.fixture
def ctx(built_lib):
    """A library context of the test's own, as the ``engine`` of the public functions: its pair counters can be read."""
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    yield types.SimpleNamespace(h=h, L=L)
    L.tcr_ctx_destroy(h)


def _pairs(ctx, entry):
    n = ctypes.c_int64(-1)
    assert getattr(ctx.L, entry + '_pairs')(ctx.h, ctypes.byref(n)) == 0
    return int(n.value)


def _in_order(monkeypatch, spoiled):
    """Order A: the front end's own.  Order B: the caller's, which is the spoiled one."""
    from tropical_cyclone_risk_amd import sitescan
    monkeypatch.undo()
    if spoiled:
        monkeypatch.setattr(sitescan, 'spatial_order', lambda lon, lat, xp: np.arange(int(lon.shape[0])))


# ---------------------------------------------------------------------------------------------------- 1. the unculled twin
# name -> (the entry point's prefix, None without a pair counter; its sphere; its records: the hazard's live samples or the track's
# (sub-)samples; the radii: 100 km and the analysis's own maximum, for the hazard 1 km too; whether it has substeps)
ANALYSES = {
    'site_hazard': ('tcr_hazard', RE_HAZARD, 'live', (1.0, 100.0, 5000.0), False),
    'site_wind-unit': ('tcr_windfield', RE_OTHERS, 'track', (100.0, 2000.0), True),
    'site_wind': ('tcr_windfield', RE_OTHERS, 'track', (100.0, 2000.0), True),
    'portfolio_loss': (None, RE_OTHERS, 'track', (100.0, 2000.0), True),
    'site_rain-total': ('tcr_rainfall', RE_OTHERS, 'track', (100.0, 2000.0), True),
    'site_rain-peak-rate': ('tcr_rainfall', RE_OTHERS, 'track', (100.0, 2000.0), True),
    'site_compound': ('tcr_compound', RE_OTHERS, 'track', (100.0, 2000.0), True),
    'site_duration': ('tcr_duration', RE_OTHERS, 'track', (100.0, 2000.0), True),
    'site_directional_wind': ('tcr_directional', RE_OTHERS, 'track', (100.0, 2000.0), True),
    'site_accumulation': ('tcr_accumulation', RE_OTHERS, 'track', (100.0, 2000.0), True),
    'site_closest_approach': ('tcr_approach', RE_OTHERS, 'track', (100.0, 5000.0), True)}


def _call(name, P, S, R, sub, ctx, value, v_half):
    """One call of the analysis with the search radius R and every optional plane."""
    from tropical_cyclone_risk_amd import accumulation, approach, compound, directional, duration, hazard, loss, rainfall, windfield
    lon, lat, groups, slon, slat = P['lon'], P['lat'], P['groups'], S['lon'], S['lat']
    kw = dict(engine=ctx, n_groups=G.N_GROUPS)
    if name == 'site_hazard':
        return hazard.site_hazard(lon, lat, P['vmax'], groups, slon, slat, radius_km=R, thresholds=THR, return_max=True, **kw)
    if name.startswith('site_wind'):
        return windfield.site_wind(lon, lat, P['v'], P['env'], groups, slon, slat, DT, ck_cd=1.0 if name.endswith('unit') else 0.9,
                                   r_out_km=R, substeps=sub, thresholds=THR, return_max=True, **kw)
    if name == 'portfolio_loss':
        return loss.portfolio_loss(lon, lat, P['v'], P['env'], groups, slon, slat, value, DT, v_half=v_half, r_out_km=R, substeps=sub,
                                   thresholds=THR, **kw)
    if name.startswith('site_rain'):
        stat = name[len('site_rain-'):]
        return rainfall.site_rain(lon, lat, P['vmax'], groups, slon, slat, DT, stat=stat, r_out_km=R, substeps=sub,
                                  thresholds=RTHR if stat == 'total' else PTHR, return_values=True, **kw)
    if name == 'site_compound':         # the wind's and the rain's own radius: the larger (the cull's) is R, once each way
        rw, rr = (R, 0.6 * R) if R <= 100.0 else (0.75 * R, R)
        return compound.site_compound(lon, lat, P['v'], P['vmax'], P['env'], groups, slon, slat, DT, THR, RTHR, wind_r_out_km=rw,
                                      rain_r_out_km=rr, substeps=sub, return_values=True, **kw)
    if name == 'site_duration':
        return duration.site_duration(lon, lat, P['v'], P['env'], groups, slon, slat, DT, levels=[20.0, 35.0], thresholds=[1.0, 3.0, 6.0],
                                      r_out_km=R, substeps=sub, return_hours=True, **kw)
    if name == 'site_directional_wind':
        return directional.site_directional_wind(lon, lat, P['v'], P['env'], groups, slon, slat, DT, n_sector=8, sector0_deg=10.0,
                                                 thresholds=THR, r_out_km=R, substeps=sub, return_max=True, **kw)
    if name == 'site_accumulation':
        return accumulation.site_accumulation(lon, lat, P['vmax'], groups, slon, slat, DT, windows_h=(1.0, 3.0, 6.0), thresholds=RTHR,
                                              return_values=True, r_out_km=R, substeps=sub, **kw)
    bands = (0.25 * R, 0.5 * R, R)
    return approach.site_closest_approach(lon, lat, P['vmax'], groups, slon, slat, DT, bands_km=bands, thresholds=THR, substeps=sub,
                                          return_planes=True, **kw)


def _flat(r):
    """a result's arrays by name, the planes of a dict of planes under their own names"""
    out = {}
    for k, a in r.items():
        if isinstance(a, dict):
            out.update({'%s[%s]' % (k, kk): aa for kk, aa in a.items()})
        else:
            out[k] = a
    return out


@functools.lru_cache(maxsize=None)
def _records(which, sub):
    P = G.storms()
    return G.hazard_records(P) if which == 'live' else G.track_records(P, sub)


@functools.lru_cache(maxsize=None)
def _sure_pairs(which, sub, R, re_km):
    T = G.twin_sites(CLUSTERS)
    return G.sure_pairs(T['lon'], T['lat'], *_records(which, sub), R, re_km)


def test_twin_layout_preconditions():
    """What the twin relies on, stated without a GPU: every tile of the spoiled order begins with an anchor whose angle to the
    next site is within MAX_GAP of pi by the kernel's own arithmetic; the record counts the pair counters are compared with."""
    T = G.twin_sites(CLUSTERS)
    n = T['lon'].size
    assert n == 64 * (6 + CLUSTERS) and np.array_equal(np.nonzero(T['anchor'])[0], np.arange(0, n, 64))
    gap = G.anchor_gap(T['lon'], T['lat'], T['anchor'])
    assert gap.max() < MAX_GAP < 0.01 / RE_OTHERS, gap.max()               # (0.01: a hundredth of r_ang at 1 km)
    assert not np.array_equal(G.morton_order(T['lon'], T['lat']), np.arange(n))
    P = G.storms()
    live, track = G.n_records(_records('live', 1)[0]), G.n_records(_records('track', 3)[0])
    assert sorted(live[[P['cats']['n_%d' % k][0] for k in (31, 32, 33, 64, 65)]]) == [31, 32, 33, 64, 65]
    assert live[P['cats']['one_sample'][0]] == 1 and track[P['cats']['one_sample'][0]] == 0
    assert np.array_equal(track, np.where(P['n_lead'] >= 2, (P['n_lead'] - 1) * 3 + 1, 0))
    s = P['cats']['hole_both'][0]
    assert live[s] == 47 and P['n_lead'][s] == 20                           # the hazard reads past a hole, the others stop at it


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(ANALYSES))
def test_gpu_unculled_twin_is_bit_identical(built_lib, ctx, monkeypatch, name):
    entry, re_km, which, radii, has_sub = ANALYSES[name]
    P, T = G.storms(), G.twin_sites(CLUSTERS)
    n_site = T['lon'].size
    assert G.anchor_gap(T['lon'], T['lat'], T['anchor']).max() < MAX_GAP < 0.01 / re_km
    rng = np.random.default_rng(3)
    value, v_half = rng.lognormal(13.0, 1.5, n_site), rng.uniform(60.0, 80.0, n_site)
    n_in = np.bincount(P['groups'], minlength=G.N_GROUPS)
    for R in radii:
        for sub in ((1, 3) if has_sub else (1,)):
            res, pairs = {}, {}
            for order in 'AB':
                _in_order(monkeypatch, spoiled=order == 'B')
                res[order] = _flat(_call(name, P, T, R, sub, ctx, value, v_half))
                pairs[order] = _pairs(ctx, entry) if entry else None
            monkeypatch.undo()
            a, b = res['A'], res['B']
            assert set(a) == set(b)
            for k in a:
                if name == 'portfolio_loss' and k in ('event_loss', 'year_max', 'year_agg'):
                    # sums over sites and tiles, which the order rearranges: tests/test_loss.py's comparison of its site shuffle
                    more = n_in if k == 'year_agg' else 0
                    assert (np.abs(b[k] - a[k]) <= (n_site + 16 + more) * U * a[k]).all(), (k, R, sub)
                else:
                    assert _same_bits(a[k], b[k]), (k, R, sub)
            planes = [k for k, x in a.items() if getattr(x, 'ndim', 0) >= 2 and x.dtype == np.float64]
            assert name == 'portfolio_loss' or (planes and all(np.isfinite(a[k]).any() for k in planes)), (R, sub)
            if entry is None:
                continue
            full = int(G.n_records(_records(which, sub)[0]).sum()) * n_site
            sure = _sure_pairs(which, sub, R, re_km)
            print('%-22s R = %6g km, substeps %d: pairs evaluated A %11d, B %11d, A / B %.4f (in range %d)'
                  % (name, R, sub, pairs['A'], pairs['B'], pairs['A'] / pairs['B'], sure))
            assert pairs['B'] == full, (R, sub)                             # nothing culled
            assert pairs['A'] < full and (R > 100.0 or 2 * pairs['A'] <= full), (R, sub)       # culling happened
            assert sure <= pairs['A'], (R, sub)                             # and no pair in range went with it


# ------------------------------------------------------------------------------------------------- 2. the geometric edges
@functools.lru_cache(maxsize=None)
def _edges():
    P, S = G.storms(), G.part2_sites()
    return P, S, G.distances(S['lon'], S['lat'], P['lon'], P['lat'])


def _angle_deg(lon1, lat1, lon2, lat2):
    return float(np.rad2deg(G.hz_angle(G.hz_a(G.hz_terms(lon1, lat1), G.hz_terms(lon2, lat2)))))


@needs_long_double
def test_edge_layout_is_decided_by_the_reference():
    """The conditions under which the GPU comparison below means something, from the reference alone."""
    P, S, d = _edges()
    lon, lat, cats = P['lon'], P['lat'], P['cats']
    assert lon.shape == (40, G.N_T) and S['lon'].size == 11 * 64
    live = ~np.isnan(lon) & ~np.isnan(lat)
    n_live = live.sum(axis=1)
    # every edge category is there, and is what its name says
    for s in cats['pole']:
        assert abs(np.nanmax(np.abs(lat[s])) - 89.999) < 1e-9
        jump = np.abs(np.diff(lon[s][live[s]]))
        assert (jump > 0).sum() == 1 and 179.0 < jump.max() < 181.0
    assert {np.sign(lat[s, 0]) for s in cats['pole']} == {1.0, -1.0}
    for s in cats['dateline']:
        x = lon[s][live[s]]
        assert x.min() < 180.0 < x.max() and np.abs(np.diff(x)).max() < 1.0
    for s in cats['dateline_pm180']:
        x = lon[s][live[s]]
        assert x.min() < -170.0 and x.max() > 179.0 and np.abs(np.diff(x)).max() > 350.0
    assert all((lat[s][live[s]] == 0.0).all() for s in cats['equator'])
    assert any(set(lon[s][live[s]]) == {0.0, 360.0} for s in cats['greenwich'])
    assert any(lon[s][live[s]].min() < 360.0 < lon[s][live[s]].max() for s in cats['greenwich'])
    assert any(lon[s][live[s]].min() < 0.0 < lon[s][live[s]].max() for s in cats['greenwich'])
    s = cats['stationary'][0]
    assert n_live[s] > 1 and len(set(lon[s][live[s]])) == 1 and len(set(lat[s][live[s]])) == 1
    assert n_live[cats['one_sample'][0]] == 1
    for s in cats['long_arc']:
        assert _angle_deg(lon[s, 0], lat[s, 0], lon[s, 64], lat[s, 64]) > 90.0
    assert [int(n_live[cats['n_%d' % k][0]]) for k in (31, 32, 33, 64, 65)] == [31, 32, 33, 64, 65]
    for k in ('hole_both', 'hole_lat'):
        s = cats[k][0]
        first = int(np.argmin(live[s]))
        assert 0 < first < n_live[s] and live[s][first + 1:].any()           # live samples on both sides of the hole
    s = cats['hole_vmax'][0]
    assert np.isnan(P['vmax'][s][live[s]]).sum() == 2 and not np.isnan(P['vmax'][s, 40])
    C = G.sites()['cats']
    SL, SA = G.sites()['lon'], G.sites()['lat']
    assert len(C['north_pole']) >= 3 and (SA[list(C['north_pole'])] == 90.0).all() and len(set(SL[list(C['north_pole'])])) >= 3
    assert len(C['south_pole']) >= 3 and (SA[list(C['south_pole'])] == -90.0).all() and len(set(SL[list(C['south_pole'])])) >= 3
    for k, x in (('lon_m180', -180.0), ('lon_180', 180.0), ('lon_0', 0.0), ('lon_360', 360.0)):
        assert len(C[k]) >= 1 and (SL[list(C[k])] == x).all()
    for i, j in zip(C['duplicate'], range(4)):
        assert SA[i] == SA[j] and abs((SL[i] - SL[j] + 180.0) % 360.0 - 180.0) < 1e-9
    assert {round(SL[i] - SL[j]) for i, j in zip(C['duplicate'], range(4))} >= {0, 360} or \
        {round(SL[i] - SL[j]) for i, j in zip(C['duplicate'], range(4))} >= {0, -360}     # in both conventions
    rl, ra = G.hazard_records(P)
    on = [(SL[i], SA[i]) for i in C['on_record']]
    assert len(on) >= 3 and all(((rl == x) & (ra == y)).any() for x, y in on) and any(abs(y - 89.999) < 1e-9 for _, y in on)
    for R in G.RADII:
        assert len(C['near_%g' % R]) >= 40
    assert len(C['scattered']) == 64 and S['scattered'].sum() == 64 and not S['anchor'][S['scattered']].any()
    sc = np.nonzero(S['scattered'])[0]
    spread = max(_angle_deg(S['lon'][sc[0]], S['lat'][sc[0]], S['lon'][i], S['lat'][i]) for i in sc)
    assert 120.0 < spread <= 150.0 and np.deg2rad(spread) + 1000.0 / 6378.0 + 0.2 < np.pi     # a large cap; up to 1000 km it is short
    # of the pi early-out for every cap of less than 0.2 rad (every segment's but the long arcs')
    # the anchored tiles
    assert np.array_equal(np.nonzero(S['anchor'])[0], np.arange(0, 6 * 64, 64))
    assert G.anchor_gap(S['lon'], S['lat'], S['anchor']).max() < MAX_GAP < 0.01 / RE_HAZARD
    for R in G.RADII:
        m, amb = G.site_max(d, P['vmax'], R)
        inside, _ = G.decide(d, R)
        touched = amb.any(axis=2)
        n_max = int((~np.isnan(m)).sum())
        print('R = %6g km: %6d pairs in range, %3d ambiguous (all at planted sites), %5d maxima, %d of them touched'
              % (R, int(inside.sum()), int(amb.sum()), n_max, int(touched.sum())))
        assert not amb[~S['planted']].any()                                 # nothing undecided but what was planted
        assert amb[S['planted']].any()
        assert touched.sum() <= 0.05 * m.size
        assert n_max >= 50
        assert G.tile_far_of_some_storm(S['lon'], S['lat'], d, R)           # order A has something to cull
        # the rim tile of R in order B: its cap without R stays (RIM_REACH R) short of the stationary storm, whose cap has radius
        # 0, and its second site is within R of it.  The pair is kept by the R in the tile cap's radius alone
        t, st = S['rim'][R], cats['stationary'][0]
        rho = float(G.distance_km(S['lon'][t:t + 64], S['lat'][t:t + 64], S['lon'][t], S['lat'][t]).max())
        assert d.km[t, st, 0] - rho > 0.9 * R and 0.9 * R < d.km[t + 1, st, 0] < R and inside[t + 1, st, :20].all() and m[t + 1, st] > 0


@needs_long_double
@pytest.mark.gpu
@pytest.mark.parametrize('R', G.RADII)
def test_gpu_hazard_edges_against_long_double(built_lib, ctx, monkeypatch, R):
    from tropical_cyclone_risk_amd import hazard
    P, S, d = _edges()
    thr = np.array([25.0, 40.0, 55.0, 70.0])
    full = int((~np.isnan(P['lon']) & ~np.isnan(P['lat'])).sum()) * S['lon'].size
    inside, _ = G.decide(d, R)
    got, pairs = {}, {}
    for order in 'AB':
        _in_order(monkeypatch, spoiled=order == 'B')
        r = hazard.site_hazard(P['lon'], P['lat'], P['vmax'], P['groups'], S['lon'], S['lat'], radius_km=R, thresholds=thr,
                               return_max=True, engine=ctx, n_groups=G.N_GROUPS)
        got[order], pairs[order] = r, _pairs(ctx, 'tcr_hazard')
    monkeypatch.undo()
    print('site_hazard, edges     R = %6g km: pairs evaluated A %8d, B %8d, A / B %.4f, all %d (in range %d)'
          % (R, pairs['A'], pairs['B'], pairs['A'] / pairs['B'], full, int(inside.sum())))
    for order in 'AB':
        r = got[order]
        ok = G.allowed(r['site_max'], d, P['vmax'], R)
        assert ok.all(), (order, [(int(i), int(s), r['site_max'][i, s]) for i, s in np.argwhere(~ok)[:5]])
        assert r['counts'].dtype == np.int32 and np.array_equal(r['counts'], HN.counts(r['site_max'], P['groups'], G.N_GROUPS, thr))
        assert not r['counts'][:, 1].any() and int(inside.sum()) <= pairs[order] <= full
    assert (~np.isnan(got['A']['site_max'])).sum() >= 50
    assert _same_bits(got['A']['site_max'], got['B']['site_max']) and _same_bits(got['A']['counts'], got['B']['counts'])
    # six tiles of B evaluate everything; the five without an anchor cull where their caps allow it
    assert pairs['A'] < full and 11 * pairs['B'] >= 6 * full
