"""Closest approach (include/tcrisk_hip.h "closest approach", tropical_cyclone_risk_amd/approach.py, csrc/tcr_approach.hip): hand
values of the NumPy restatement (tests/approach_numpy.py), the argument handling and the command line without a GPU; on the GPU
the restatement's allowed winners and payloads, the counts from the call's own planes, consistency with the site hazard,
bit-identity, the entry points and the command line."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import approach_numpy as AN
from tests import levels_numpy as LN
from tests import windfield_numpy as WN

DT = 3600.0
HEADING_TOL_DEG = 1e-9          # fp64 atan2 and the degree conversion round at ~1e-13 degrees: 10^4 times that
CROSS_REL = 1e-9                # the side's sign is exact unless |cross| <= CROSS_REL speed


# ------------------------------------------------------------------------------------------------------------------ CPU
def _line_track(n, lat0=20.0):
    """One storm of n samples moving west along lat0, a quarter of a degree per hour."""
    return (290.0 - 0.25 * np.arange(n))[None, :], np.full((1, n), lat0), np.full((1, n), 30.0)


def _restate(lon, lat, v, slon, slat, r_km, substeps=1, rmax_km=None):
    slon, slat = np.asarray(slon, float), np.asarray(slat, float)
    recs = AN.records(lon, lat, v, DT, rmax_km=rmax_km, substeps=substeps)
    ref = AN.approach(recs, slon, slat, r_km)
    return recs, ref, AN.planes(ref, recs, slon, slat, AN.hours_per_record(DT, substeps))


def _hand_sites():
    """North of sample 4 of the line track, south of it, on it, and out of reach."""
    return np.array([289.0, 289.0, 289.0, 200.0]), np.array([20.6, 19.4, 20.0, -30.0])


def _check_hand_values(P, sub):
    """What the line track of 9 samples gives at _hand_sites, in the restatement and on the GPU alike."""
    for k in AN.PLANES:
        assert P[k].shape == (4, 1) and np.isnan(P[k][3, 0]), k                # out of reach: NaN in every plane
    assert (P['heading_deg'][:3, 0] == 270.0).all()                           # due west, exactly
    assert P['time_h'][:3, 0].tolist() == [4.0, 4.0, 4.0]                      # record 4 sub: sample 4, hours since the first
    assert P['side_km'][0, 0] > 0 and P['side_km'][0, 0] == P['distance_km'][0, 0]     # north of a westward track: on the right
    assert P['side_km'][1, 0] < 0 and P['side_km'][1, 0] == -P['distance_km'][1, 0]    # the mirror case: on the left
    assert abs(P['distance_km'][0, 0] - WN.haversine_km(289.0, 20.0, 289.0, 20.6)) < 1e-9
    assert P['distance_km'][2, 0] == 0.0 and P['side_km'][2, 0] == 0.0         # on a sample
    assert (P['v'][:3, 0] == 30.0).all()
    assert np.allclose(P['rmax_km'][:3, 0], 46.4 * np.exp(-0.0155 * 30.0 + 0.0169 * 20.0), rtol=1e-13)
    speed = AN.RE_M * np.cos(np.deg2rad(20.0)) * np.deg2rad(0.25) / DT
    assert np.allclose(P['speed'][:3, 0], speed, rtol=1e-13)


def test_restatement_hand_values():
    lon, lat, v = _line_track(9)
    slon, slat = _hand_sites()
    for sub in (1, 4):
        recs, ref, P = _restate(lon, lat, v, slon, slat, 200.0, substeps=sub)
        assert recs[0].shape == (8, 8 * sub + 1)
        assert ref['inc_any'][:, 0].tolist() == [True, True, True, False] and np.array_equal(ref['inc_any'], ref['inc_sure'])
        assert ref['first'][:, 0].tolist() == [4 * sub, 4 * sub, 4 * sub, -1] and ref['n_allowed'][:3, 0].tolist() == [1, 1, 1]
        _check_hand_values(P, sub)
    # the southern hemisphere changes nothing about right and left
    lon_s, lat_s, v_s = _line_track(9, lat0=-20.0)
    _, _, Ps = _restate(lon_s, lat_s, v_s, [289.0, 289.0], [-19.4, -20.6], 200.0)
    assert Ps['side_km'][0, 0] > 0 and Ps['side_km'][1, 0] < 0 and (Ps['heading_deg'] == 270.0).all()
    # a stationary segment: no heading, no side, speed 0; the records of the segments around it have theirs
    lon2 = lon.copy()
    lon2[0, 5:] = lon2[0, 4:-1]                                             # samples 4 and 5 are one point
    _, ref2, P2 = _restate(lon2, lat, v, [lon2[0, 4]], [20.3], 200.0)
    assert ref2['first'][0, 0] == 4 and ref2['n_allowed'][0, 0] == 2         # records 4 and 5 tie: the earlier one
    assert np.isnan(P2['heading_deg'][0, 0]) and P2['speed'][0, 0] == 0.0 and P2['side_km'][0, 0] == 0.0
    assert P2['distance_km'][0, 0] > 30.0
    # a one-sample track has no records; neither has one with a bad rm
    lon1 = lon.copy()
    lon1[0, 1] = np.nan
    recs1, ref1, P1 = _restate(lon1, lat, v, slon, slat, 200.0)
    assert recs1[0] is None and not ref1['inc_any'].any() and all(np.isnan(P1[k]).all() for k in AN.PLANES)
    rm = np.full(lon.shape, 30.0)
    rm[0, 3] = 0.0
    assert AN.records(lon, lat, v, DT, rmax_km=rm)[0] is None and AN.records(lon, lat, v, DT, rmax_km=30.0)[0][3].tolist() == [30.0] * 9


def _tie_track():
    """Along the equator, samples at +-0.25 and +-0.75 degrees of the site (0, 0): records 1 and 2 are equally far, bit for bit."""
    return np.array([[0.75, 0.25, -0.25, -0.75]]), np.zeros((1, 4)), np.array([[20.0, 30.0, 40.0, 50.0]])


def test_restatement_tie_takes_the_earlier_record():
    lon, lat, v = _tie_track()
    _, ref, P = _restate(lon, lat, v, [0.0], [0.0], 100.0)
    assert ref['q'][0][0, 1] == ref['q'][0][0, 2] and ref['first'][0, 0] == 1 and ref['n_allowed'][0, 0] == 2
    assert P['time_h'][0, 0] == 1.0 and P['v'][0, 0] == 30.0 and P['side_km'][0, 0] == 0.0      # on the track: no side


def test_restatement_counts():
    d = np.array([[10.0, 60.0, np.nan, 150.0, 50.0]])
    v = np.array([[40.0, 20.0, np.nan, 33.0, 33.0]])
    c = AN.counts(d, v, np.array([0, 0, 0, 2, 2]), 3, [50.0, 100.0, 200.0], [20.0, 33.0, 34.0])
    assert c.shape == (1, 3, 3, 3) and c.dtype == np.int32
    assert c[0, 0].tolist() == [[1, 1, 1], [2, 1, 1], [2, 1, 1]] and not c[0, 1].any()
    assert c[0, 2].tolist() == [[1, 1, 0], [1, 1, 0], [2, 2, 0]]             # distance == band and v == threshold count


def test_return_periods_and_defaults():
    from tropical_cyclone_risk_amd import approach
    assert approach.PLANES == AN.PLANES and approach.DEFAULT_BANDS_KM == (50., 100., 200.)
    assert approach.hours_per_record(3600.0, 4) == 0.25 == AN.hours_per_record(3600.0, 4)
    c = np.zeros((2, 3, 2, 2), np.int32)
    c[0, 0, 0] = [2, 0]
    c[0, 2, 0] = [3, 0]
    c[1, 1, 1] = [4, 1]
    rp = approach.return_periods(c, 30)
    assert rp.shape == (2, 2, 2)
    assert rp[0].tolist() == [[6.0, np.inf], [np.inf, np.inf]] and rp[1].tolist() == [[np.inf, np.inf], [7.5, 30.0]]
    with pytest.raises(ValueError):
        approach.return_periods(c[:, 0], 30)
    assert approach.wanted_planes(True) == list(AN.PLANES) and approach.wanted_planes(None) == []
    assert approach.wanted_planes(['v', 'distance_km']) == ['distance_km', 'v']


def test_argument_errors_before_any_device_work():
    from tropical_cyclone_risk_amd import approach
    rng = np.random.default_rng(0)
    lon, lat, v = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    base = dict(lon=lon, lat=lat, v=v, groups=np.zeros(3, np.int64), site_lon=np.array([280.0]), site_lat=np.array([20.0]), dt_s=DT)
    bad = [dict(bands_km=[100.0, 50.0]), dict(bands_km=[50.0, 50.0]), dict(bands_km=[0.0, 50.0]), dict(bands_km=[-5.0]),
           dict(bands_km=[np.nan]), dict(bands_km=[50.0, np.inf]), dict(bands_km=[50.0, 5000.5]), dict(bands_km=[]),
           dict(bands_km=np.arange(1.0, 10.0)),                                       # more than 8
           dict(bands_km=[50.0, 100.0, 200.0], thresholds=np.arange(1.0, 23.0)),      # 3 * 22 = 66 cells
           dict(bands_km=np.arange(1.0, 9.0), thresholds=np.arange(1.0, 9.0)),        # 8 * 9 = 72 cells
           dict(thresholds=[3.0, 1.0]), dict(thresholds=[]), dict(thresholds=[1.0, np.inf]),
           dict(return_planes=['nope']), dict(return_planes=['v', 'v']), dict(return_planes='v'), dict(return_planes=[0]),
           dict(substeps=0), dict(substeps=65), dict(substeps=1.5), dict(dt_s=0.0), dict(dt_s=np.inf), dict(rmax_km=-5.0),
           dict(rmax_km=np.nan), dict(rmax_km=np.full((3, 4), 20.0)), dict(v=v[:, :4]), dict(groups=np.zeros(2, np.int64)),
           dict(site_lat=np.array([np.nan])), dict(site_lon=np.array([1.0, 2.0])), dict(groups=np.array([0, 1, 2]), n_groups=2),
           dict(n_groups=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            approach.site_closest_approach(**dict(base, **kw))
    # the limits themselves pass the checks: 8 * 8 and 1 * 64 cells, a band of 5000 km
    approach._check_bands(np.arange(1.0, 9.0), np.arange(1.0, 8.0))
    approach._check_bands([5000.0], np.arange(1.0, 64.0))


def test_cli_arguments(capsys):
    from tropical_cyclone_risk_amd import approach
    a = approach.parse_args(['x.nc', '--site', '1,2'])
    assert a.bands.tolist() == [50.0, 100.0, 200.0] and np.array_equal(a.thresholds, approach.DEFAULT_THRESHOLDS)
    assert a.substeps == 1 and a.rmax_km is None and a.planes == [] and a.out == 'approach.npz'
    assert not hasattr(a, 'return_periods') and not hasattr(a, 'events_out')
    b = approach.parse_args(['x.nc', '--grid', '270:271:0.5,20:21:1', '--bands', '50,100,200', '--thresholds', '20:70:10',
                             '--substeps', '4', '--planes', 'heading_deg,distance_km', '--out', 'a.npz'])
    assert b.bands.tolist() == [50.0, 100.0, 200.0] and b.thresholds.tolist() == [20, 30, 40, 50, 60, 70] and b.substeps == 4
    assert b.planes == ['distance_km', 'heading_deg'] and b.out == 'a.npz'
    for argv in (['x.nc'], ['x.nc', '--site', '1,2', '--bands', '100,50'], ['x.nc', '--site', '1,2', '--bands', 'a,b'],
                 ['x.nc', '--site', '1,2', '--bands', '6000'], ['x.nc', '--site', '1,2', '--planes', 'nope'],
                 ['x.nc', '--site', '1,2', '--substeps', '0'], ['x.nc', '--site', '1,2', '--return-periods', '10'],
                 ['x.nc', '--site', '1,2', '--thresholds', '1:70:1']):
        with pytest.raises(SystemExit):
            approach.parse_args(argv)
    capsys.readouterr()


def test_approach_symbols_exported(built_lib):
    from tropical_cyclone_risk_amd import _lib
    assert os.path.samefile(built_lib, _lib.LIB_PATH)
    L = _lib.lib()                                                      # (the package's own way in: one HIP runtime per process)
    for name in ('tcr_approach_dev', 'tcr_approach_host', 'tcr_approach_pairs'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.tcr_abi_version() == 7 and _lib.APPROACH_PLANES == len(AN.PLANES)


# ------------------------------------------------------------------------------------------------------------------ GPU
# substeps, rm (None: Willoughby, a constant, 'plane'), bands (1, 3 and 8 rows), n_bin: 3 * 16, 1 * 64, 8 * 8 and 3 * 6 cells
CASES = [(1, None, (50.0, 100.0, 200.0), 15),
         (3, 35.0, (150.0,), 63),
         (6, 'plane', (25.0, 50.0, 75.0, 100.0, 150.0, 200.0, 300.0, 500.0), 7),
         (3, 'plane', (60.0, 120.0, 400.0), 5)]
SEEDS = [300, 301, 302, 303]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs of CASES[i] and the restatement on them (computed once, never changed)."""
    from tests.test_duration import _sites, _tracks
    sub, rm, bands, n_bin = CASES[i]
    rng, lon, lat, v, _, groups, n_groups = _tracks(SEEDS[i])
    if isinstance(rm, str):
        rm = rng.uniform(8.0, 90.0, lon.shape)
    slon, slat = _sites(rng, lon, lat, bands[-1])
    thr = np.linspace(5.0, 75.0, n_bin)
    unit = AN.hours_per_record(DT, sub)
    recs = AN.records(lon, lat, v, DT, rmax_km=rm, substeps=sub)
    ref = AN.approach(recs, slon, slat, bands[-1])
    own = AN.planes(ref, recs, slon, slat, unit)
    for a in list(own.values()) + [x for x in ref['q'] if x is not None] + [ref[k] for k in ref if k != 'q']:
        a.setflags(write=False)
    kw = dict(bands_km=np.array(bands), thresholds=thr, rmax_km=rm, substeps=sub, n_groups=n_groups)
    return dict(tracks=(lon, lat, v, groups), sites=(slon, slat), kw=kw, unit=unit, recs=recs, ref=ref, own=own, n_groups=n_groups)


def _condition(d):
    """What makes a case a test: (share of the possibly included cells with a single allowed winner, storms per band, cells with
    the site on the right, on the left)."""
    ref, own = d['ref'], d['own']
    cells = ref['inc_any']
    with np.errstate(invalid='ignore'):
        per_band = [int((own['distance_km'] <= b).sum()) for b in d['kw']['bands_km']]
        right, left = int((own['side_km'] > 0).sum()), int((own['side_km'] < 0).sum())
    return (ref['n_allowed'][cells] == 1).sum() / cells.sum(), per_band, right, left


@pytest.mark.parametrize('i', range(len(CASES)))
def test_cases_are_decided_by_the_restatement(i):
    """Not a measurement: the cases are chosen so that nearly every cell has one allowed winner, every band holds storms and the
    sites lie on both sides of the tracks."""
    d = _case(i)
    share, per_band, right, left = _condition(d)
    print('case %d: %.4f of the cells have one allowed winner; storms per band %s; right %d, left %d' % (i, share, per_band, right, left))
    assert share >= 0.95 and min(per_band) >= 50 and right >= 50 and left >= 50
    assert d['sites'][0].size % 64 != 0 and d['sites'][0].size > 64
    assert d['ref']['n_edge'].sum() >= 5                                    # sites planted at exactly the outer radius
    assert sum(r is None for r in d['recs']) >= 2                           # tracks of one sample in lon, lat and v


@functools.lru_cache(maxsize=None)
def _gpu(i):
    from tropical_cyclone_risk_amd import approach
    d = _case(i)
    lon, lat, v, groups = d['tracks']
    return approach.site_closest_approach(lon, lat, v, groups, d['sites'][0], d['sites'][1], DT, return_planes=True, **d['kw'])


def _indices(time_h, unit):
    """The record indices behind a time_h plane, which must reproduce it bit for bit; -1 where it is NaN."""
    nan = np.isnan(time_h)
    idx = np.where(nan, -1, np.rint(np.where(nan, 0.0, time_h) / unit)).astype(np.int64)
    assert LN.same_bits(time_h, np.where(nan, np.nan, idx.astype(np.float64) * unit))
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(CASES)))
def test_gpu_matches_restatement(built_lib, i):
    d, r = _case(i), _gpu(i)
    ref, recs, unit = d['ref'], d['recs'], d['unit']
    slon, slat = d['sites']
    P = r['planes']
    assert tuple(P) == AN.PLANES and np.array_equal(r['bands_km'], d['kw']['bands_km'])
    idx = _indices(P['time_h'], unit)
    nan = idx < 0
    assert not (nan & ref['inc_sure']).any() and not (~nan & ~ref['inc_any']).any()      # between inc_sure and inc_any
    for k in AN.PLANES:
        assert P[k].shape == nan.shape
        if k != 'heading_deg':
            assert np.array_equal(np.isnan(P[k]), nan), k                   # NaN in every plane alike
    assert np.isnan(P['heading_deg'][nan]).all()
    worst_heading, n_checked, n_undecided = 0.0, 0, 0
    for s, rec in enumerate(recs):
        hit = np.nonzero(~nan[:, s])[0]
        if rec is None:
            assert hit.size == 0
        if rec is None or hit.size == 0:
            continue
        ix = idx[hit, s]
        assert (ix < rec.shape[1]).all()
        assert AN.allowed(ref, s, hit, ix).all(), (s, hit[~AN.allowed(ref, s, hit, ix)][:5])
        vals, cross, speed = AN.payload(rec, slon[hit], slat[hit], ix, unit)
        for name, want in zip(AN.PLANES, vals):
            got = P[name][hit, s]
            if name == 'heading_deg':
                assert np.array_equal(np.isnan(got), np.isnan(want))
                ok = ~np.isnan(want)
                if ok.any():
                    worst_heading = max(worst_heading, float(np.abs((got[ok] - want[ok] + 180.0) % 360.0 - 180.0).max()))
                assert ((got[ok] >= 0.0) & (got[ok] < 360.0)).all()
            elif name == 'side_km':
                decided = np.abs(cross) > CROSS_REL * speed
                n_undecided += int((~decided).sum())
                assert np.array_equal(np.sign(got[decided]), np.sign(want[decided]))
                assert (WN.close(np.abs(got), vals[0]) | (~decided & (got == 0.0))).all()
            else:
                assert WN.close(got, want).all(), (name, s)
        n_checked += hit.size
    print('case %d: %d cells checked, heading off by at most %.3g degrees, %d cells with an undecided side'
          % (i, n_checked, worst_heading, n_undecided))
    assert worst_heading <= HEADING_TOL_DEG and n_checked > 300
    single = ~nan & (ref['n_allowed'] == 1)
    assert np.array_equal(idx[single], ref['first'][single])                # one allowed winner: that one


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(CASES)))
def test_gpu_counts_from_own_planes(built_lib, i):
    d, r = _case(i), _gpu(i)
    groups, n_groups = d['tracks'][3], d['n_groups']
    P = r['planes']
    assert r['counts'].dtype == np.int32 and r['counts'].shape == (d['sites'][0].size, n_groups, len(CASES[i][2]), CASES[i][3])
    assert np.array_equal(r['counts'], AN.counts(P['distance_km'], P['v'], groups, n_groups, r['bands_km'], r['thresholds']))
    assert r['counts'].sum() > 100
    assert (np.diff(r['counts'], axis=3) <= 0).all() and (np.diff(r['counts'], axis=2) >= 0).all()      # monotone in bin and in band
    for g in (1, 4):                                                    # the empty groups
        assert not r['counts'][:, g].any()


@pytest.mark.gpu
def test_gpu_hand_values(built_lib):
    from tropical_cyclone_risk_amd import approach
    lon, lat, v = _line_track(9)
    slon, slat = _hand_sites()
    for sub in (1, 4):
        r = approach.site_closest_approach(lon, lat, v, np.zeros(1, np.int64), slon, slat, DT, bands_km=[50.0, 200.0], substeps=sub,
                                           thresholds=[30.0, 30.5], return_planes=True)
        _check_hand_values(r['planes'], sub)
        assert r['counts'][:, 0].tolist() == [[[0, 0], [1, 0]], [[0, 0], [1, 0]], [[1, 0], [1, 0]], [[0, 0], [0, 0]]]
    # a tie goes to the earlier record, whichever way the track runs
    lon_t, lat_t, v_t = _tie_track()
    for flip, want_v in ((False, 30.0), (True, 40.0)):
        sl = slice(None, None, -1) if flip else slice(None)
        r = approach.site_closest_approach(lon_t[:, sl], lat_t, v_t[:, sl], np.zeros(1, np.int64), [0.0], [0.0], DT, bands_km=[100.0],
                                           return_planes=True)
        P = r['planes']
        assert P['time_h'][0, 0] == 1.0 and P['v'][0, 0] == want_v and P['side_km'][0, 0] == 0.0
        assert P['heading_deg'][0, 0] == (90.0 if flip else 270.0)
    # a stationary segment
    lon2 = lon.copy()
    lon2[0, 5:] = lon2[0, 4:-1]
    P2 = approach.site_closest_approach(lon2, lat, v, np.zeros(1, np.int64), [lon2[0, 4]], [20.3], DT, return_planes=True)['planes']
    assert P2['time_h'][0, 0] == 4.0 and np.isnan(P2['heading_deg'][0, 0]) and P2['speed'][0, 0] == 0.0 and P2['side_km'][0, 0] == 0.0
    assert P2['distance_km'][0, 0] > 30.0
    # a one-sample track; a track with a bad rm
    lon1 = lon.copy()
    lon1[0, 1] = np.nan
    rm = np.full(lon.shape, 30.0)
    rm[0, 3] = 0.0
    for kw in (dict(lon=lon1), dict(lon=lon, rmax_km=rm)):
        r = approach.site_closest_approach(lat=lat, v=v, groups=np.zeros(1, np.int64), site_lon=slon, site_lat=slat, dt_s=DT,
                                           return_planes=True, **kw)
        assert all(np.isnan(r['planes'][k]).all() for k in AN.PLANES) and not r['counts'].any()


@pytest.mark.gpu
def test_gpu_consistent_with_the_site_hazard(built_lib):
    """At the same angular radius, the intensity at the closest point is one of the intensities the hazard takes the max of."""
    from tropical_cyclone_risk_amd import hazard
    d, r = _case(0), _gpu(0)                                            # substeps 1: the records are the samples
    lon, lat, v, groups = d['tracks']
    slon, slat = d['sites']
    n = AN.track_length(lon, lat, v)
    cut = (np.arange(lon.shape[1])[None, :] >= n[:, None]) | (n[:, None] < 2)       # the approach's track rule, as NaN tails
    lon_c, lat_c, v_c = (np.where(cut, np.nan, a) for a in (lon, lat, v))
    radius = float(d['kw']['bands_km'][-1]) * 6378.0 / AN.RE_KM         # the hazard's sphere has 6378 km
    m = hazard.site_hazard(lon_c, lat_c, v_c, groups, slon, slat, radius_km=radius, thresholds=d['kw']['thresholds'],
                           return_max=True, n_groups=d['n_groups'])['site_max']
    v_cpa = r['planes']['v']
    both = ~np.isnan(v_cpa) & ~np.isnan(m)
    assert both.sum() > 300 and (v_cpa[both] <= m[both]).all() and (v_cpa[both] < m[both]).sum() > 100
    amb = d['ref']['inc_any'] & ~d['ref']['inc_sure']
    assert np.array_equal(np.isnan(v_cpa)[~amb], np.isnan(m)[~amb])


@pytest.mark.gpu
def test_gpu_bit_identical_across_runs_site_order_and_storm_order(built_lib):
    from tropical_cyclone_risk_amd import approach
    d, a = _case(2), _gpu(2)
    lon, lat, v, groups = d['tracks']
    slon, slat = d['sites']
    rng = np.random.default_rng(5)
    kw = dict(d['kw'], return_planes=True)

    def same(x, y, sites=slice(None), storms=slice(None)):
        for k in AN.PLANES:
            assert np.array_equal(x['planes'][k].view(np.int64), np.ascontiguousarray(y['planes'][k][sites][:, storms]).view(np.int64)), k
        assert np.array_equal(x['counts'], y['counts'][sites])
    same(approach.site_closest_approach(lon, lat, v, groups, slon, slat, DT, **kw), a)
    ps = rng.permutation(slon.size)
    same(approach.site_closest_approach(lon, lat, v, groups, slon[ps], slat[ps], DT, **kw), a, sites=ps)
    pt = rng.permutation(lon.shape[0])                                  # storms shuffled within and across groups
    same(approach.site_closest_approach(lon[pt], lat[pt], v[pt], groups[pt], slon, slat, DT, **dict(kw, rmax_km=kw['rmax_km'][pt])), a,
         storms=pt)


@pytest.mark.gpu
def test_gpu_host_and_device_entry_points_agree(built_lib):
    import types
    import torch
    from tropical_cyclone_risk_amd import _lib, approach
    d, ref = _case(3), _gpu(3)
    lon, lat, v, groups = d['tracks']
    slon, slat = d['sites']
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(x, device=dev) for x in [lon, lat, v, slon, slat, d['kw']['rmax_km']]]
    h = ctypes.c_void_p()
    assert _lib.lib().tcr_ctx_create(0, ctypes.byref(h)) == 0
    eng = types.SimpleNamespace(h=h)                                    # one context, so one workspace, for the three calls
    side = torch.cuda.Stream(dev)
    try:
        for want in (True, ['side_km', 'time_h'], False):
            with torch.cuda.stream(side):
                r = approach.site_closest_approach(t[0], t[1], t[2], groups, t[3], t[4], DT, engine=eng, return_planes=want,
                                                   **dict(d['kw'], rmax_km=t[5]))
            side.synchronize()
            assert r['counts'].device == dev and np.array_equal(r['counts'].cpu().numpy(), ref['counts'])
            names = approach.wanted_planes(want)
            assert list(r['planes']) == names                               # the planes not asked for are absent
            for k in names:
                assert r['planes'][k].device == dev and LN.same_bits(r['planes'][k].cpu().numpy(), ref['planes'][k]), k
    finally:
        side.synchronize()
        _lib.lib().tcr_ctx_destroy(h)
    # some of the planes through the host entry point: the others are absent, and nothing else moves
    part = approach.site_closest_approach(lon, lat, v, groups, slon, slat, DT, return_planes=['rmax_km', 'heading_deg'], **d['kw'])
    assert list(part['planes']) == ['heading_deg', 'rmax_km'] and np.array_equal(part['counts'], ref['counts'])
    for k in part['planes']:
        assert LN.same_bits(part['planes'][k], ref['planes'][k])
    none = approach.site_closest_approach(lon, lat, v, groups, slon, slat, DT, **d['kw'])
    assert none['planes'] == {} and np.array_equal(none['counts'], ref['counts'])
    # no storms at all
    e = approach.site_closest_approach(lon[:0], lat[:0], v[:0], groups[:0], slon, slat, DT, return_planes=True,
                                       **dict(d['kw'], n_groups=2, rmax_km=None))
    assert all(e['planes'][k].shape == (slon.size, 0) for k in AN.PLANES) and e['counts'].shape == (slon.size, 2, 3, 5)
    assert not e['counts'].any()


@pytest.mark.gpu
def test_gpu_abi_outputs_optional_bad_arguments_and_pairs(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    assert L.tcr_abi_version() == 7
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        n_trk, n_t, n_site = 3, 9, 2
        planes = [np.full((n_trk, n_t), x) for x in (280.0, 20.0, 30.0)]
        planes[0] = planes[0] - 0.25 * np.arange(n_t) + 0.5 * np.arange(n_trk)[:, None]
        planes[2] = planes[2] + np.arange(n_t)
        for p in planes:
            p[2, 4:] = np.nan                                           # a track of four samples
        off = (ctypes.c_int64 * 3)(0, 2, n_trk)
        slon, slat = np.array([279.5, 281.0]), np.array([20.5, 19.6])
        bands0, thr0 = np.array([60.0, 120.0, 400.0]), np.array([10.0, 32.0, 36.0])
        rm_plane = np.full((n_trk, n_t), 25.0)
        trk = _lib.HazardTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=planes[0].ctypes.data, lat=planes[1].ctypes.data,
                                vmax=planes[2].ctypes.data, n_group=2, group_off=off)

        def call(bands=bands0, thr=thr0, want=range(7), no_array=False, rmax=None, **p):
            prm = _lib.ApproachParams(**dict(dict(dt_s=DT, substeps=1, rmax_const_km=0.0), **p))
            n_band, n_bin = len(bands), len(thr)
            counts = np.full((n_site, 2, max(n_band, 1), max(n_bin, 1)), -7, np.int32)
            out = np.full((7, n_site, n_trk), -7.0)
            arr = (ctypes.c_void_p * 7)()
            for k in want:
                arr[k] = out[k].ctypes.data
            bd, th = np.asarray(bands, float), np.asarray(thr, float)
            rc = L.tcr_approach_host(h, ctypes.byref(trk), None if rmax is None else rmax.ctypes.data, ctypes.byref(prm), n_site,
                                     slon.ctypes.data, slat.ctypes.data, n_band, bd.ctypes.data_as(_lib.DP), n_bin,
                                     th.ctypes.data_as(_lib.DP), counts.ctypes.data, None if no_array else arr)
            return rc, counts, out
        rc, counts, out = call()
        assert rc == 0 and counts.sum() > 0 and (counts >= 0).all() and not np.isnan(out).any()
        assert np.array_equal(counts, AN.counts(out[0], out[2], np.array([0, 0, 1]), 2, bands0, thr0))
        assert (out[1, :, 2] <= 3.0).all()                              # the short track ends at its fourth sample
        pairs, hpairs = ctypes.c_int64(), ctypes.c_int64()
        assert L.tcr_approach_pairs(h, ctypes.byref(pairs)) == 0 and pairs.value > 0
        # outputs left out: the others are what they were, and nothing is written where nothing was asked for
        for kw in (dict(want=(1, 5)), dict(want=()), dict(no_array=True)):
            rc, c2, o2 = call(**kw)
            assert rc == 0 and np.array_equal(c2, counts), kw
            for k in range(7):
                assert np.array_equal(o2[k], out[k]) if (k in kw.get('want', ()) and not kw.get('no_array')) else (o2[k] == -7).all()
        # the rm rules: a constant, a plane
        assert np.all(call(rmax_const_km=40.0)[2][6] == 40.0) and np.all(call(rmax=rm_plane)[2][6] == 25.0)
        # the site hazard evaluates the same pairs at the same angular radius (substeps 1: the records are its samples)
        hc = np.zeros((n_site, 2, 3), np.int32)
        assert L.tcr_hazard_host(h, ctypes.byref(trk), n_site, slon.ctypes.data, slat.ctypes.data, 400.0 * 6378.0 / AN.RE_KM, 3,
                                 thr0.ctypes.data_as(_lib.DP), hc.ctypes.data, None) == 0
        assert L.tcr_hazard_pairs(h, ctypes.byref(hpairs)) == 0 and hpairs.value == pairs.value
        assert np.array_equal(hc >= counts[:, :, 2], np.ones_like(hc, bool))       # the max within R is at least the CPA's v
        bad = [dict(bands=[100.0, 50.0]), dict(bands=[0.0, 50.0]), dict(bands=[50.0, np.nan]), dict(bands=[5000.5]), dict(bands=[]),
               dict(bands=np.arange(1.0, 10.0), thr=[1.0]), dict(thr=[3.0, 1.0]), dict(thr=[np.inf]), dict(thr=[]),
               dict(bands=[1.0, 2.0, 3.0], thr=np.arange(1.0, 23.0)), dict(bands=np.arange(1.0, 9.0), thr=np.arange(1.0, 9.0)),
               dict(substeps=0), dict(substeps=65), dict(dt_s=0.0), dict(rmax_const_km=-1.0), dict(rmax_const_km=np.nan),
               dict(rmax=rm_plane, rmax_const_km=30.0)]
        for kw in bad:
            assert call(**kw)[0] == -1, kw
            assert L.tcr_last_error(h).startswith(b'tcr_approach:'), (kw, L.tcr_last_error(h))
        assert call(bands=np.arange(1.0, 9.0) * 50.0, thr=np.arange(1.0, 8.0), want=())[0] == 0       # 64 cells
        none = ctypes.c_void_p()
        assert L.tcr_approach_pairs(h, None) == -1 and L.tcr_approach_pairs(none, ctypes.byref(pairs)) == -1
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_cli_round_trip(built_lib, tmp_path, capsys):
    from tests.test_levels import _write_track_file
    from tropical_cyclone_risk_amd import analysis, approach
    fn = _write_track_file(tmp_path, np.random.default_rng(5))
    sites = ['--site=-75.0,24.0', '--site', '286.5,25.5', '--site=-72.25,27.0', '--site', '10.0,50.0']
    opts = ['--bands', '50,100,200', '--thresholds', '20:70:10', '--substeps', '4']
    keys = {'counts', 'return_period', 'bands_km', 'thresholds', 'site_lon', 'site_lat', 'total_years', 'dt_s', 'substeps', 'rmax_km',
            'group_file', 'group_year', 'files'}
    out = str(tmp_path / 'approach.npz')
    assert approach.main([fn, '--out', out] + sites + opts) == 0
    plain = np.load(out)
    assert set(plain.files) == keys
    text = capsys.readouterr().out
    assert 'passages at or above' in text and 'return period (years) of a passage' in text
    lon, lat, vmax, groups, gfile, gyear, more = analysis.load_groups([fn], extra=('time',))
    dt = analysis.sample_spacing(more['time'])
    api = approach.site_closest_approach(lon, lat, vmax, groups, plain['site_lon'], plain['site_lat'], dt, bands_km=[50.0, 100.0, 200.0],
                                         thresholds=np.arange(20.0, 71.0, 10.0), substeps=4, n_groups=3, return_planes=True)
    assert int(plain['total_years']) == 3 and float(plain['dt_s']) == dt and plain['bands_km'].tolist() == [50.0, 100.0, 200.0]
    assert np.array_equal(plain['counts'], api['counts']) and api['counts'].sum() > 0 and plain['counts'].shape == (4, 3, 3, 6)
    assert np.array_equal(plain['return_period'], approach.return_periods(api['counts'], 3)) and plain['return_period'].shape == (4, 3, 6)
    assert not plain['counts'][3].any() and np.isinf(plain['return_period'][3]).all()
    assert approach.main([fn, '--out', out, '--planes', 'distance_km,heading_deg'] + sites + opts) == 0
    z = np.load(out)
    assert set(z.files) == keys | {'distance_km', 'heading_deg'}
    for k in ('distance_km', 'heading_deg'):
        assert LN.same_bits(z[k], api['planes'][k])
    assert np.array_equal(z['counts'], plain['counts'])
