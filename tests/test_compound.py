"""Compound wind-rain hazard (tropical_cyclone_risk_amd/compound.py, csrc/tcr_compound.hip): joint exceedance counts of the wind
footprint and the rainfall footprint at sites, from one scan.  CPU tests pin the NumPy counting (tests/compound_numpy.py) by
hand and check the argument handling; GPU tests (`-m gpu`) check the two planes bit for bit against the single-hazard entry
points, the table exactly against the counting of the call's own planes, both against the restatements, and the order
guarantee."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import compound_numpy as CN
from tests import rainfall_numpy as RN
from tests import test_rainfall as TR
from tests import windfield_numpy as WN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 3600.0
WTHR = np.array([8.0, 16.0, 24.0, 32.0, 40.0, 48.0])                      # m/s
RTHR = {'total': np.array([5.0, 25.0, 50.0, 100.0, 150.0, 200.0, 300.0]),  # mm
        'peak-rate': np.array([0.5, 1.0, 2.0, 4.0, 6.0, 8.0, 10.0])}       # mm/h: (6 + 1) x (7 + 1) = 56 cells
RKEY = {'total': 'site_rain', 'peak-rate': 'site_peak_rate'}
PARENT_RKEY = {'total': 'site_total', 'peak-rate': 'site_peak_rate'}
NAN, INF = float('nan'), float('inf')


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_joint_counts_by_hand():
    wthr, rthr = np.array([20.0, 30.0]), np.array([50.0, 100.0, 200.0])
    #             storm 0      1       2      3     4      5
    W = np.array([[25.0,    NAN,   30.0,  NAN,  45.0,  10.0]])     # ranks 1 0 2 0 2 0  (30.0 equals a threshold: it passes it)
    P = np.array([[120.0,  60.0,   NAN,   NAN,  250.0, 50.0]])     # ranks 2 1 0 0 3 1  (50.0 likewise)
    groups, n_groups = np.array([0, 0, 0, 2, 2, 2]), 4              # groups 1 and 3 are empty
    assert CN.rank(W, wthr).tolist() == [[1, 0, 2, 0, 2, 0]] and CN.rank(P, rthr).tolist() == [[2, 1, 0, 0, 3, 1]]
    c = CN.joint_counts(W, P, groups, n_groups, wthr, rthr)
    assert c.shape == (1, 4, 3, 4) and c.dtype == np.int32
    assert c[0, 0].tolist() == [[3, 2, 1, 0],       # a = 0: all three; P >= 50: storms 0, 1; >= 100: storm 0
                                [2, 1, 1, 0],       # W >= 20: storms 0, 2; and P >= 50 / 100: storm 0 (storm 2 has no rain)
                                [1, 0, 0, 0]]       # W >= 30: storm 2 alone, which has no rain
    assert c[0, 2].tolist() == [[3, 2, 1, 1],       # storm 3 (NaN on both) only in the corner; P >= 50: storms 4, 5
                                [1, 1, 1, 1],       # W >= 20: storm 4
                                [1, 1, 1, 1]]
    assert (c[0, 1] == 0).all() and (c[0, 3] == 0).all()
    # the identities of the contract
    assert np.array_equal(c[..., 1:, 0], WN.counts(W, groups, n_groups, wthr))
    assert np.array_equal(c[..., 0, 1:], RN.counts(P, groups, n_groups, rthr))
    assert c[0, :, 0, 0].tolist() == [3, 0, 3, 0]
    o = CN.or_counts(c)
    assert o.shape == (1, 4, 2, 3)
    assert np.array_equal(o, c[..., 1:, :1] + c[..., :1, 1:] - c[..., 1:, 1:])
    assert o[0, 0].tolist() == [[3, 2, 2], [3, 2, 1]] and o[0, 2].tolist() == [[2, 1, 1], [2, 1, 1]]
    with np.errstate(invalid='ignore'):
        for a in range(2):
            for b in range(3):
                either = (W >= wthr[a]) | (P >= rthr[b])
                assert o[0, 0, a, b] == either[0, :3].sum() and o[0, 2, a, b] == either[0, 3:].sum()
    from tropical_cyclone_risk_amd import compound
    assert np.array_equal(compound.or_counts(c), o)
    rp = compound.table_return_periods(o, 4)
    assert rp.shape == (1, 2, 3) and rp[0, 0].tolist() == [4 / 5, 4 / 3, 4 / 3]


def test_track_length_and_cut():
    a = np.arange(12.0).reshape(2, 6)
    b = a.copy()
    b[0, 4], b[1, 0] = np.nan, np.inf
    assert CN.track_length([a, b]).tolist() == [4, 0] and CN.track_length([a, a]).tolist() == [6, 6]
    c = CN.cut(a, [4, 0])
    assert np.array_equal(c[0, :4], a[0, :4]) and np.isnan(c[0, 4:]).all() and np.isnan(c[1]).all()


def _small(rng):
    lon, lat, vmax = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    env = [rng.normal(0, 5, (3, 5)) for _ in range(4)]
    return dict(lon=lon, lat=lat, v=0.8 * vmax, vmax=vmax, env=env, groups=np.zeros(3, np.int64), site_lon=np.array([280.0]),
                site_lat=np.array([20.0]), dt_s=DT, wind_thresholds=np.array([10.0, 20.0]), rain_thresholds=np.array([10.0, 50.0]))


def test_argument_errors_before_any_device_work(monkeypatch):
    from tropical_cyclone_risk_amd import _lib, compound, rainfall

    def no_library():
        raise AssertionError('the library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', no_library)
    base = _small(np.random.default_rng(0))
    a0, b0 = rainfall.DEFAULT_COEFFICIENTS
    rm_bad = np.full((3, 5), 30.0)
    rm_bad[1, 2] = 0.0
    bad = [dict(wind_thresholds=np.arange(1.0, 8.0), rain_thresholds=np.arange(1.0, 9.0)),              # 8 x 9 = 72 cells
           dict(wind_thresholds=np.arange(1.0, 33.0), rain_thresholds=np.array([1.0, 2.0])),           # 33 x 3 = 99
           dict(wind_thresholds=np.array([])), dict(rain_thresholds=np.array([])),
           dict(wind_thresholds=np.array([20.0, 10.0])), dict(rain_thresholds=np.array([50.0, 50.0])),
           dict(wind_thresholds=np.array([10.0, np.nan])), dict(rain_thresholds=np.array([10.0, np.inf])),
           dict(vmax=base['vmax'][:, :4]), dict(vmax=base['vmax'][:2]),
           # the footprint's
           dict(env=base['env'][:3]), dict(ck_cd=2.0), dict(ck_cd=0.0), dict(wind_r_out_km=0.0), dict(wind_r_out_km=2000.5),
           dict(rmax_km=-1.0), dict(rmax_km=rm_bad), dict(rmax_km=np.ones((3, 4))), dict(v=base['v'][:, :4]),
           # the rainfall's
           dict(stat='sum'), dict(rain_r_out_km=np.nan), dict(rain_r_out_km=2001.0), dict(v_hi_kt=170.0), dict(v_lo_kt=0.0),
           dict(coefficients=(a0, b0[:3])), dict(coefficients=((-1.10, -6.0, 64.5, 150.0), b0)),
           # common
           dict(substeps=0), dict(substeps=65), dict(substeps=1.5), dict(dt_s=0.0), dict(dt_s=np.inf),
           dict(groups=np.zeros(2, np.int64)), dict(groups=np.array([0, -1, 0])), dict(site_lat=np.array([np.nan])),
           dict(site_lon=np.array([1.0, 2.0])), dict(groups=np.array([0, 1, 2]), n_groups=2), dict(n_groups=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            compound.site_compound(**dict(base, **kw))
    # good arguments do reach the library: the largest table, a plane of rm, both statistics, different radii
    for kw in (dict(), dict(wind_thresholds=np.arange(1.0, 8.0), rain_thresholds=np.arange(1.0, 8.0)),
               dict(wind_thresholds=np.array([10.0]), rain_thresholds=np.arange(1.0, 32.0)),
               dict(rmax_km=np.full((3, 5), 30.0), stat='peak-rate', wind_r_out_km=200.0, return_values=True)):
        with pytest.raises(AssertionError, match='the library was touched'):
            compound.site_compound(**dict(base, **kw))


def test_cli_arguments():
    from tropical_cyclone_risk_amd import analysis, compound
    a = compound.parse_args(['x.nc', '--site=-80.19,25.76', '--grid', '270:271:0.5,20:21:1', '--wind-thresholds', '20:50:10',
                             '--rain-thresholds', '50:200:50', '--wind-r-out-km', '300', '--rain-r-out-km', '600', '--substeps', '4'])
    assert a.wind_r_out_km == 300.0 and a.rain_r_out_km == 600.0 and a.substeps == 4 and a.stat == 'total' and a.out == 'compound.npz'
    assert np.array_equal(a.wind_thresholds, [20, 30, 40, 50]) and np.array_equal(a.rain_thresholds, [50, 100, 150, 200])
    assert analysis.collect_sites(a)[0].size == 7
    b = compound.parse_args(['x.nc', 'y.nc', '--site', '1,2'])
    assert b.tracks == ['x.nc', 'y.nc'] and b.wind_r_out_km == 500.0 and b.rain_r_out_km == 500.0 and b.substeps == 1
    assert np.array_equal(b.wind_thresholds, compound.DEFAULT_WIND_THRESHOLDS)
    assert np.array_equal(b.rain_thresholds, compound.DEFAULT_RAIN_THRESHOLDS)
    assert (b.wind_thresholds.size + 1) * (b.rain_thresholds.size + 1) <= compound.MAX_CELLS
    c = compound.parse_args(['x.nc', '--site', '1,2', '--stat', 'peak-rate', '--rain-thresholds', '2:10:2', '--out', 'p.npz'])
    assert c.stat == 'peak-rate' and np.array_equal(c.rain_thresholds, [2, 4, 6, 8, 10]) and c.out == 'p.npz'
    for argv in (['x.nc'], ['x.nc', '--site', '1,2', '--stat', 'peak-rate'], ['x.nc', '--site', '1,2', '--stat', 'mean'],
                 ['x.nc', '--site', '1,2', '--wind-thresholds', '10:80:5'],                       # 16 x 9 cells
                 ['x.nc', '--site', '1,2', '--thresholds', '10:80:5']):
        with pytest.raises(SystemExit):
            compound.parse_args(argv)


def test_compound_symbols_exported_and_abi_version_unchanged(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_compound_dev', 'tcr_compound_host', 'tcr_compound_pairs'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    L.tcr_abi_version.restype = ctypes.c_int
    assert L.tcr_abi_version() == 7 and _lib.TCR_ABI_VERSION == 7
    hdr = open(os.path.join(ROOT, 'include', 'tcrisk_hip.h')).read()
    for name in ('tcr_compound_dev', 'tcr_compound_host', 'tcr_compound_pairs'):
        assert 'int %s(' % name in hdr


# ------------------------------------------------------------------------------------------------------- shared inputs
@functools.lru_cache(maxsize=None)
def _inputs(seed, r_site):
    """test_rainfall's stress set (140 storms x 48 samples: 0, 1, 2, 33, 34 samples, one far storm, both conventions across the
    dateline; 70 sites; empty groups) with env planes that are finite everywhere and v = 0.8 vmax: all eight planes are finite
    exactly where the rainfall's three are, so both parents see the compound's track.  Shared: callers must not write to it."""
    rng = np.random.default_rng(seed)
    lon, lat, vmax = TR._stress_tracks(rng)
    n_trk, n_t = lon.shape
    groups, n_groups = TR._groups(rng, n_trk)
    slon, slat = TR._stress_sites(rng, lon, lat, vmax, r_site)
    env = tuple(rng.normal(0, 8, (n_trk, n_t)) for _ in range(4))
    v = 0.8 * vmax
    assert np.array_equal(CN.track_length((lon, lat, v, vmax) + env), RN.track_length(lon, lat, vmax))
    for a in (lon, lat, vmax, v, slon, slat, groups) + env:
        a.setflags(write=False)
    return lon, lat, v, vmax, env, groups, n_groups, slon, slat


RESTATED = [(3, 'total', 0.9, 400.0, 400.0), (1, 'peak-rate', 1.0, 300.0, 400.0)]       # sub, stat, ck_cd, wind r_out, rain r_out
RESTATED_SEED = 41


@functools.lru_cache(maxsize=None)
def _restated(sub, stat, c, rw, rr):
    """The two planes by the NumPy restatements on the shared track, after asserting that the inputs decide every count: no
    (site, record) pair in either r_out band, no value within the tolerance of a threshold."""
    lon, lat, v, vmax, env, groups, n_groups, slon, slat = _inputs(RESTATED_SEED, 400.0)
    n8 = CN.track_length((lon, lat, v, vmax) + env)
    wrec = WN.samples(lon, lat, v, list(env) + [vmax], DT, substeps=sub)               # (the extra plane only cuts the track)
    W, amb_any, _ = WN.site_max(wrec, slon, slat, rw, c)
    assert not amb_any.any() and not WN.undecided(W, amb_any, WTHR).any()
    P, n_band = RN.site_values(RN.records(lon, lat, CN.cut(vmax, n8), DT, sub), slon, slat, rr, stat)
    assert n_band == 0 and not RN.near_threshold(P, RTHR[stat]).any()
    return W, P


@pytest.mark.parametrize('cfg', RESTATED)
def test_restated_inputs_decide_every_count(cfg):
    """What the GPU comparison against the restatements rests on, checked without a GPU."""
    W, P = _restated(*cfg)
    assert (~np.isnan(W)).sum() > 200 and (~np.isnan(P)).sum() > 300
    c = CN.joint_counts(W, P, *_inputs(RESTATED_SEED, 400.0)[5:7], WTHR, RTHR[cfg[1]])
    assert c[..., 1:, 1:].sum() > 100                                                   # the joint table is not trivially empty


# ------------------------------------------------------------------------------------------------------------------ GPU
def _t(x, dev):
    import torch
    return torch.as_tensor(np.array(x), device=dev)                        # (a copy: the shared inputs are read-only)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _compound(inp, stat, sub, c, rw, rr, **kw):
    from tropical_cyclone_risk_amd import compound
    lon, lat, v, vmax, env, groups, n_groups, slon, slat = inp
    kw.setdefault('return_values', True)
    return compound.site_compound(lon, lat, v, vmax, env, groups, slon, slat, DT, WTHR, RTHR[stat], ck_cd=c, wind_r_out_km=rw,
                                  rain_r_out_km=rr, substeps=sub, stat=stat, n_groups=n_groups, **kw)


def _parents(inp, stat, sub, c, rw, rr, vmax=None):
    from tropical_cyclone_risk_amd import rainfall, windfield
    lon, lat, v, vmax0, env, groups, n_groups, slon, slat = inp
    w = windfield.site_wind(lon, lat, v, env, groups, slon, slat, DT, ck_cd=c, r_out_km=rw, substeps=sub, thresholds=WTHR,
                            return_max=True, n_groups=n_groups)
    r = rainfall.site_rain(lon, lat, vmax0 if vmax is None else vmax, groups, slon, slat, DT, stat=stat, r_out_km=rr, substeps=sub,
                           thresholds=RTHR[stat], return_values=True, n_groups=n_groups)
    return w, r


def _same_as_parents(res, w, r, stat):
    assert np.array_equal(_bits(res['site_wind']), _bits(w['site_max']))
    assert np.array_equal(_bits(res[RKEY[stat]]), _bits(r[PARENT_RKEY[stat]]))
    assert np.array_equal(res['counts'][..., 1:, 0], w['counts']) and np.array_equal(res['counts'][..., 0, 1:], r['counts'])


def _exact_table(res, inp, stat):
    groups, n_groups = inp[5:7]
    want = CN.joint_counts(res['site_wind'], res[RKEY[stat]], groups, n_groups, WTHR, RTHR[stat])
    assert res['counts'].shape == want.shape and res['counts'].dtype == np.int32
    assert np.array_equal(res['counts'], want)
    assert np.array_equal(res['counts'][..., 0, 0], np.broadcast_to(np.bincount(groups, minlength=n_groups), want.shape[:2]))


@pytest.mark.gpu
@pytest.mark.parametrize('sub,stat,c', [(1, 'total', 1.0), (3, 'total', 0.9), (1, 'peak-rate', 0.9), (3, 'peak-rate', 1.0)])
def test_gpu_bits_against_the_parents_and_exact_table(built_lib, sub, stat, c):
    """Both planes and both marginals are the single-hazard entry points' bit for bit, the table is the
    NumPy counting of the call's own planes, and it does not depend on whether the planes are asked for."""
    inp = _inputs(17, 400.0)
    res = _compound(inp, stat, sub, c, 400.0, 400.0)
    w, r = _parents(inp, stat, sub, c, 400.0, 400.0)
    _same_as_parents(res, w, r, stat)
    _exact_table(res, inp, stat)
    assert (~np.isnan(res['site_wind'])).sum() > 300 and res['counts'][..., 1:, 1:].sum() > 100
    assert np.isnan(res['site_wind'][:, :2]).all() and np.isnan(res['site_wind'][:, TR.FAR]).all()
    assert np.isnan(res[RKEY[stat]][:, :2]).all() and np.isnan(res[RKEY[stat]][:, TR.FAR]).all()
    bare = _compound(inp, stat, sub, c, 400.0, 400.0, return_values=False)
    assert set(bare) == {'counts', 'wind_thresholds', 'rain_thresholds'} and np.array_equal(bare['counts'], res['counts'])


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', RESTATED)
def test_gpu_matches_the_restatements(built_lib, cfg):
    sub, stat, c, rw, rr = cfg
    W, P = _restated(*cfg)
    inp = _inputs(RESTATED_SEED, 400.0)
    res = _compound(inp, stat, sub, c, rw, rr)
    for name, got, want, close in (('wind', res['site_wind'], W, WN.close), ('rain', res[RKEY[stat]], P, RN.close)):
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        print('%s: %d values, largest |got - want| = %.3g' % (name, (~np.isnan(want)).sum(), np.nanmax(np.abs(got - want))))
        assert close(got, want).all(), name
    assert np.array_equal(res['counts'], CN.joint_counts(W, P, inp[5], inp[6], WTHR, RTHR[stat]))


@pytest.mark.gpu
def test_gpu_different_radii(built_lib):
    inp = _inputs(17, 400.0)
    groups, n_groups = inp[5:7]
    for stat in ('total', 'peak-rate'):
        res = _compound(inp, stat, 2, 0.9, 200.0, 500.0)
        w, r = _parents(inp, stat, 2, 0.9, 200.0, 500.0)
        _same_as_parents(res, w, r, stat)
        _exact_table(res, inp, stat)
        W, P = res['site_wind'], res[RKEY[stat]]
        only_rain = np.isnan(W) & ~np.isnan(P)
        assert only_rain.sum() > 50 and not (np.isnan(P) & ~np.isnan(W)).any()       # the wind's disc lies inside the rain's
        # those storms alone: counted on the rain axis under "no condition on the wind", and in no row with one
        alone = CN.joint_counts(np.where(only_rain, W, np.nan), np.where(only_rain, P, np.nan), groups, n_groups, WTHR, RTHR[stat])
        rest = CN.joint_counts(np.where(only_rain, np.nan, W), np.where(only_rain, np.nan, P), groups, n_groups, WTHR, RTHR[stat])
        assert (alone[..., 1:, :] == 0).all() and alone[..., 0, 1:].sum() > 0
        assert np.array_equal(res['counts'][..., 1:, :], rest[..., 1:, :])
        assert np.array_equal(res['counts'][..., 0, 1:], rest[..., 0, 1:] + alone[..., 0, 1:])


def _dev_call(L, h, t, vmax, rmax, slon, slat, groups_off, sub, n_trk, n_t, stream=None):
    """tcr_compound_dev on torch planes already grouped (one group): (counts, site_wind, site_rain) tensors."""
    import torch
    from tropical_cyclone_risk_amd import _lib
    dev = t[0].device
    off = (ctypes.c_int64 * 2)(*groups_off)
    trk = _lib.WindTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=t[0].data_ptr(), lat=t[1].data_ptr(), v=t[2].data_ptr(),
                          u250=t[3].data_ptr(), v250=t[4].data_ptr(), u850=t[5].data_ptr(), v850=t[6].data_ptr(),
                          rmax_km=None if rmax is None else rmax.data_ptr(), n_group=1, group_off=off)
    wp = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=400.0, rmax_const_km=0.0, substeps=sub)
    rp = _lib.RainParams(dt_s=DT, r_out_km=400.0, v_lo_kt=35.0, v_hi_kt=155.0, a=(ctypes.c_double * 4)(*RN.DEFAULT_A),
                         b=(ctypes.c_double * 4)(*RN.DEFAULT_B), substeps=sub, stat=0)
    n_site = slon.shape[0]
    counts = torch.empty((n_site, 1, WTHR.size + 1, RTHR['total'].size + 1), dtype=torch.int32, device=dev)
    sw, sr = (torch.empty((n_site, n_trk), dtype=torch.float64, device=dev) for _ in range(2))
    rc = L.tcr_compound_dev(h, ctypes.byref(trk), vmax.data_ptr(), ctypes.byref(wp), ctypes.byref(rp), n_site, slon.data_ptr(),
                            slat.data_ptr(), WTHR.size, WTHR.ctypes.data_as(_lib.DP), RTHR['total'].size,
                            RTHR['total'].ctypes.data_as(_lib.DP), counts.data_ptr(), sw.data_ptr(), sr.data_ptr(), stream)
    assert rc == 0, L.tcr_last_error(h)
    torch.cuda.synchronize(dev)
    return counts.cpu().numpy(), sw.cpu().numpy(), sr.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _cut_storms():
    """Two storms of _inputs(17) with all 48 samples whose cuts must show: a has samples from 20 on within 350 km of a site (its
    rain there loses terms), b is within 350 km of some site only from sample 31 on (its wind there becomes NaN)."""
    lon, lat, v, vmax, env, groups, n_groups, slon, slat = _inputs(17, 400.0)
    full = np.nonzero(RN.track_length(lon, lat, vmax) == lon.shape[1])[0]
    reach = {int(s): RN.haversine_km(lon[s][None, :], lat[s][None, :], slon[:, None], slat[:, None]) <= 350.0 for s in full}
    a = next(s for s in reach if reach[s][:, 20:].any())
    b = next(s for s in reach if s != a and (reach[s][:, 31:].any(axis=1) & ~reach[s][:, :31].any(axis=1)).any())
    return a, b


def test_cut_storms_exist():
    a, b = _cut_storms()
    assert a != b


@pytest.mark.gpu
def test_gpu_eight_plane_track_rule(built_lib):
    import torch
    from tropical_cyclone_risk_amd import _lib
    lon, lat, v, vmax, env, groups, n_groups, slon, slat = _inputs(17, 400.0)
    inp = _inputs(17, 400.0)
    n_trk, n_t = lon.shape
    a, b = _cut_storms()
    # a NaN in an env plane at sample 20 of storm a (lon, lat, vmax finite beyond it) cuts the rain of that storm too
    env_cut = [e.copy() for e in env]
    env_cut[2][a, 20] = np.nan
    # a NaN in vmax alone at sample 30 of storm b cuts its wind
    vmax_cut = vmax.copy()
    vmax_cut[b, 30] = np.nan
    cut_inp = (lon, lat, v, vmax_cut, tuple(env_cut), groups, n_groups, slon, slat)
    res = _compound(cut_inp, 'total', 3, 0.9, 400.0, 400.0)
    n8 = CN.track_length((lon, lat, v, vmax_cut) + tuple(env_cut))
    assert n8[a] == 20 and n8[b] == 30
    # each parent on planes truncated to the shared track
    trunc = (lon, lat, CN.cut(v, n8), vmax_cut, tuple(env_cut), groups, n_groups, slon, slat)
    w, r = _parents(trunc, 'total', 3, 0.9, 400.0, 400.0, vmax=CN.cut(vmax_cut, n8))
    _same_as_parents(res, w, r, 'total')
    _exact_table(res, cut_inp, 'total')
    # ... which is not what they give on the uncut planes: the cut changed values of both storms
    w0, r0 = _parents(inp, 'total', 3, 0.9, 400.0, 400.0)
    assert not np.array_equal(_bits(r0['site_total'][:, a]), _bits(res['site_rain'][:, a]))
    assert not np.array_equal(_bits(w0['site_max'][:, b]), _bits(res['site_wind'][:, b]))
    others = np.setdiff1d(np.arange(n_trk), [a, b])
    assert np.array_equal(_bits(r0['site_total'][:, others]), _bits(res['site_rain'][:, others]))
    assert np.array_equal(_bits(w0['site_max'][:, others]), _bits(res['site_wind'][:, others]))

    # a bad rmax_km sample through _dev: the storm is dropped, NaN on both planes; the other storms are what a good plane gives
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        t = [_t(x, dev) for x in (lon, lat, v) + env]
        tv, sl, sa = (_t(x, dev) for x in (vmax, slon, slat))
        rm = np.full((n_trk, n_t), 35.0)
        good = _dev_call(L, h, t, tv, torch.as_tensor(rm, device=dev), sl, sa, (0, n_trk), 2, n_trk, n_t)
        rm[a, 5] = np.nan
        bad = _dev_call(L, h, t, tv, torch.as_tensor(rm, device=dev), sl, sa, (0, n_trk), 2, n_trk, n_t)
        assert not np.isnan(good[1][:, a]).all() and not np.isnan(good[2][:, a]).all()
        assert np.isnan(bad[1][:, a]).all() and np.isnan(bad[2][:, a]).all()
        rest = np.setdiff1d(np.arange(n_trk), [a])
        assert np.array_equal(_bits(bad[1][:, rest]), _bits(good[1][:, rest]))
        assert np.array_equal(_bits(bad[2][:, rest]), _bits(good[2][:, rest]))
        one = np.zeros(n_trk, np.int64)
        assert np.array_equal(bad[0], CN.joint_counts(bad[1], bad[2], one, 1, WTHR, RTHR['total']))
        assert (bad[0][:, 0, 0, 0] == n_trk).all()
        # _host rejects the same plane
        p = lambda x: np.ascontiguousarray(x).ctypes.data                                 # noqa: E731
        keep = [np.ascontiguousarray(x) for x in (lon, lat, v) + env + (vmax, rm, slon, slat)]
        off = (ctypes.c_int64 * 2)(0, n_trk)
        trk = _lib.WindTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=p(keep[0]), lat=p(keep[1]), v=p(keep[2]), u250=p(keep[3]),
                              v250=p(keep[4]), u850=p(keep[5]), v850=p(keep[6]), rmax_km=p(keep[8]), n_group=1, group_off=off)
        wp = _lib.WindParams(dt_s=DT, ck_cd=1.0, r_out_km=400.0, rmax_const_km=0.0, substeps=2)
        rp = _lib.RainParams(dt_s=DT, r_out_km=400.0, v_lo_kt=35.0, v_hi_kt=155.0, a=(ctypes.c_double * 4)(*RN.DEFAULT_A),
                             b=(ctypes.c_double * 4)(*RN.DEFAULT_B), substeps=2, stat=0)
        counts = np.zeros((slon.size, 1, WTHR.size + 1, RTHR['total'].size + 1), np.int32)
        rc = L.tcr_compound_host(h, ctypes.byref(trk), p(keep[7]), ctypes.byref(wp), ctypes.byref(rp), slon.size, p(keep[9]), p(keep[10]),
                                 WTHR.size, WTHR.ctypes.data_as(_lib.DP), RTHR['total'].size, RTHR['total'].ctypes.data_as(_lib.DP),
                                 counts.ctypes.data, None, None)
        assert rc == -1 and L.tcr_last_error(h).decode().startswith('tcr_compound_host: rmax_km must be finite and > 0')
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_bit_identical_across_runs_site_order_storm_order_and_site_count(built_lib):
    import torch
    from tropical_cyclone_risk_amd import compound
    lon, lat, v, vmax, env, groups, n_groups, slon, slat = _inputs(5, 500.0)
    n_trk = lon.shape[0]
    rng = np.random.default_rng(55)
    dev = torch.device('cuda', 0)
    tl, ta, tv, tm, sl, sa = (_t(x, dev) for x in (lon, lat, v, vmax, slon, slat))
    te = [_t(e, dev) for e in env]

    def same(x, y):
        return torch.equal(x.view(torch.int64), y.view(torch.int64))                   # bits: NaN equal to NaN
    for stat in ('total', 'peak-rate'):
        key = RKEY[stat]

        def run(idx=None, g=groups, lon_s=sl, lat_s=sa):
            pl = [tl, ta, tv, tm] + te if idx is None else [x[idx] for x in [tl, ta, tv, tm] + te]
            return compound.site_compound(pl[0], pl[1], pl[2], pl[3], pl[4:], g, lon_s, lat_s, DT, WTHR, RTHR[stat], ck_cd=0.9,
                                          wind_r_out_km=300.0, rain_r_out_km=500.0, substeps=3, stat=stat, return_values=True,
                                          n_groups=n_groups)

        def equal(x, y, cols=None, rows=None):
            for k in ('site_wind', key):
                want = y[k] if cols is None else y[k][:, cols]
                want = want if rows is None else want[rows]
                assert same(x[k], want), k
        a = run()
        assert (~torch.isnan(a[key])).sum() > 500 and (~torch.isnan(a['site_wind'])).sum() > 300
        b = run()
        equal(b, a)
        assert torch.equal(a['counts'], b['counts'])
        ps = torch.as_tensor(rng.permutation(slon.size), device=dev)
        c = run(lon_s=sl[ps], lat_s=sa[ps])
        equal(c, a, rows=ps)
        assert torch.equal(c['counts'], a['counts'][ps])
        pt = np.arange(n_trk)                                               # storms permuted within their groups
        for g in range(n_groups):
            i = np.nonzero(groups == g)[0]
            pt[i] = rng.permutation(i)
        assert np.array_equal(groups[pt], groups) and not np.array_equal(pt, np.arange(n_trk))
        tp = torch.as_tensor(pt, device=dev)
        d = run(idx=tp)
        equal(d, a, cols=tp)
        assert torch.equal(d['counts'], a['counts'])
        px = rng.permutation(n_trk)                                         # ... and across groups, the groups going along
        tx = torch.as_tensor(px, device=dev)
        e = run(idx=tx, g=groups[px])
        equal(e, a, cols=tx)
        assert torch.equal(e['counts'], a['counts'])
        # 200 far sites more: other tiles, another grid, the same 70 rows
        fl_ = torch.as_tensor(rng.uniform(0.0, 40.0, 200), device=dev)
        fa_ = torch.as_tensor(rng.uniform(55.0, 80.0, 200), device=dev)
        f = run(lon_s=torch.cat([sl, fl_]), lat_s=torch.cat([sa, fa_]))
        for k in ('site_wind', key):
            assert same(f[k][:70], a[k]) and torch.isnan(f[k][70:]).all()
        assert torch.equal(f['counts'][:70], a['counts'])
        size = torch.as_tensor(np.bincount(groups, minlength=n_groups), device=dev, dtype=torch.int32)
        assert torch.equal(f['counts'][70:, :, 0, 0], size.expand(200, -1))
        mask = torch.ones_like(f['counts'][70:], dtype=torch.bool)
        mask[:, :, 0, 0] = False
        assert int(f['counts'][70:][mask].sum()) == 0


@pytest.mark.gpu
def test_gpu_entry_points_pairs_no_storms_and_three_streams(built_lib):
    import torch
    from tropical_cyclone_risk_amd import _lib, compound, rainfall, windfield
    from tropical_cyclone_risk_amd.engine import TCEngine
    lon, lat, v, vmax, env, groups, n_groups, slon, slat = _inputs(8, 400.0)
    dev = torch.device('cuda', 0)
    tl, ta, tv, tm, sl, sa = (_t(x, dev) for x in (lon, lat, v, vmax, slon, slat))
    te = [_t(e, dev) for e in env]
    eng = TCEngine('NA', device=0)
    L = _lib.lib()
    pairs = ctypes.c_int64(-1)
    s1, s2, s3 = (torch.cuda.Stream(dev) for _ in range(3))
    kw = dict(ck_cd=0.9, wind_r_out_km=300.0, rain_r_out_km=400.0, substeps=4, return_values=True, n_groups=n_groups, engine=eng)
    try:
        assert L.tcr_compound_pairs(eng.h, ctypes.byref(pairs)) == -1
        assert L.tcr_last_error(eng.h).decode().startswith('tcr_compound_pairs: no tcr_compound_* call')
        n_rec = sum((int(k) - 1) * 4 + 1 for k in RN.track_length(lon, lat, vmax) if k >= 2)
        for stat in ('total', 'peak-rate'):
            ref = compound.site_compound(lon, lat, v, vmax, env, groups, slon, slat, DT, WTHR, RTHR[stat], stat=stat, **kw)      # _host
            assert L.tcr_compound_pairs(eng.h, ctypes.byref(pairs)) == 0
            assert 0 < pairs.value <= n_rec * slon.size
            with torch.cuda.stream(s1):
                r = compound.site_compound(tl, ta, tv, tm, te, groups, sl, sa, DT, WTHR, RTHR[stat], stat=stat, **kw)            # _dev
            s1.synchronize()
            assert r['counts'].device == dev and r['site_wind'].device == dev and r[RKEY[stat]].device == dev
            assert np.array_equal(r['counts'].cpu().numpy(), ref['counts'])
            for k in ('site_wind', RKEY[stat]):
                assert np.array_equal(_bits(r[k].cpu().numpy()), _bits(ref[k])), k
        # no storms at all
        z = compound.site_compound(lon[:0], lat[:0], v[:0], vmax[:0], [e[:0] for e in env], groups[:0], slon, slat, DT, WTHR,
                                   RTHR['total'], return_values=True, n_groups=2, engine=eng)
        assert z['counts'].shape == (70, 2, 7, 8) and z['counts'].sum() == 0
        assert z['site_wind'].shape == (70, 0) and z['site_rain'].shape == (70, 0)
        zt = compound.site_compound(tl[:0], ta[:0], tv[:0], tm[:0], [e[:0] for e in te], groups[:0], sl, sa, DT, WTHR, RTHR['total'],
                                    n_groups=2, engine=eng)
        assert tuple(zt['counts'].shape) == (70, 2, 7, 8) and int(zt['counts'].sum()) == 0
        assert L.tcr_compound_pairs(eng.h, ctypes.byref(pairs)) == 0 and pairs.value == 0

        # the context's fifth workspace: a compound, a footprint and a rainfall call in flight on three streams
        def comp():
            return compound.site_compound(tl, ta, tv, tm, te, groups, sl, sa, DT, WTHR, RTHR['total'], **kw)

        def wind():
            return windfield.site_wind(tl, ta, tv, te, groups, sl, sa, DT, substeps=4, return_max=True, n_groups=n_groups, engine=eng)

        def rain():
            return rainfall.site_rain(tl, ta, tm, groups, sl, sa, DT, substeps=4, thresholds=TR.THR_TOTAL, return_values=True,
                                      n_groups=n_groups, engine=eng)
        c0, w0, r0 = comp(), wind(), rain()
        torch.cuda.synchronize(dev)
        for _ in range(3):
            with torch.cuda.stream(s1):
                c1 = comp()
            with torch.cuda.stream(s2):
                w1 = wind()
            with torch.cuda.stream(s3):
                r1 = rain()
            for s in (s1, s2, s3):
                s.synchronize()
            for k in ('site_wind', 'site_rain'):
                assert torch.equal(c1[k].view(torch.int64), c0[k].view(torch.int64)), k
            assert torch.equal(w1['site_max'].view(torch.int64), w0['site_max'].view(torch.int64))
            assert torch.equal(r1['site_total'].view(torch.int64), r0['site_total'].view(torch.int64))
            assert torch.equal(c1['counts'], c0['counts']) and torch.equal(w1['counts'], w0['counts'])
            assert torch.equal(r1['counts'], r0['counts'])
        assert int(c0['counts'][..., 1:, 1:].sum()) > 0 and int(w0['counts'].sum()) > 0 and int(r0['counts'].sum()) > 0
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_more_storms_in_a_chunk_than_a_histogram_cell_holds(built_lib):
    """The joint histogram's cells are 16 bits, so the scan keeps a chunk at 65 535 storms.  Without that cap this call has one
    chunk: 8192 tiles of sites leave the chunk table one piece per group, and the group has 70 000 storms.  All but the first 64
    sites are far from every storm (culled per storm: cheap), and still count every storm in the corner."""
    from tropical_cyclone_risk_amd import compound, windfield
    n_trk, n_site = 70000, 64 * 8192
    rng = np.random.default_rng(3)
    lon = 200.0 + rng.uniform(-1.0, 1.0, (n_trk, 1)) + np.array([[0.0, 0.1]])
    lat = 15.0 + rng.uniform(-1.0, 1.0, (n_trk, 1)) + np.array([[0.0, 0.1]])
    vmax = rng.uniform(20.0, 70.0, (n_trk, 2))
    env = [rng.normal(0, 8, (n_trk, 2)) for _ in range(4)]
    groups = np.zeros(n_trk, np.int64)
    slon = np.concatenate([200.0 + rng.uniform(-1.0, 1.0, 64), rng.uniform(20.0, 60.0, n_site - 64)])
    slat = np.concatenate([15.0 + rng.uniform(-1.0, 1.0, 64), rng.uniform(50.0, 70.0, n_site - 64)])
    wthr, rthr = np.array([25.0]), np.array([2.0])
    res = compound.site_compound(lon, lat, 0.8 * vmax, vmax, env, groups, slon, slat, DT, wthr, rthr, wind_r_out_km=300.0,
                                 rain_r_out_km=300.0)
    c = res['counts']
    assert c.shape == (n_site, 1, 2, 2) and (c[:, 0, 0, 0] == n_trk).all()
    assert (c[64:, 0].reshape(-1, 4)[:, 1:] == 0).all()
    w = windfield.site_wind(lon, lat, 0.8 * vmax, env, groups, slon[:64], slat[:64], DT, r_out_km=300.0, thresholds=wthr)
    assert np.array_equal(c[:64, :, 1:, 0], w['counts']) and c[:64, 0, 1, 0].min() > 1000
    assert (c[:64, 0, 0, 1] > 65535).any()                                 # every storm rains 2 mm within 150 km: past 16 bits


@pytest.mark.gpu
def test_gpu_abi_rejects_bad_arguments(built_lib):
    from tropical_cyclone_risk_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.tcr_ctx_create(0, ctypes.byref(h)) == 0
    try:
        n_trk, n_t = 2, 6
        planes = [np.full((n_trk, n_t), x) for x in (280.0, 20.0, 30.0, 3.0, -2.0, 1.0, 4.0, 38.0)]     # the seven, then vmax
        planes[0] = planes[0] + 0.1 * np.arange(n_t)
        off = (ctypes.c_int64 * 2)(0, n_trk)
        s = np.array([280.2]), np.array([20.0])
        wthr, rthr = np.arange(1.0, 66.0), np.arange(1.0, 66.0)                  # as long as any n_bin the checks read
        counts = np.zeros((1, 1, 64), np.int32)
        a0, b0 = RN.DEFAULT_A, RN.DEFAULT_B
        ptr = [x.ctypes.data for x in planes]

        def call(n_w=2, n_r=2, n_t_=n_t, vmax=ptr[7], wthr_=wthr, rthr_=rthr, a=a0, b=b0, wind=None, **rain):
            trk = _lib.WindTracks(n_trk=n_trk, n_t=n_t_, row_stride=n_t, lon=ptr[0], lat=ptr[1], v=ptr[2], u250=ptr[3], v250=ptr[4],
                                  u850=ptr[5], v850=ptr[6], rmax_km=None, n_group=1, group_off=off)
            wp = _lib.WindParams(**dict(dict(dt_s=DT, ck_cd=0.9, r_out_km=500.0, rmax_const_km=0.0, substeps=1), **(wind or {})))
            rp = _lib.RainParams(**dict(dict(dt_s=DT, r_out_km=500.0, v_lo_kt=35.0, v_hi_kt=155.0, a=(ctypes.c_double * 4)(*a),
                                             b=(ctypes.c_double * 4)(*b), substeps=1, stat=0), **rain))
            return L.tcr_compound_host(h, ctypes.byref(trk), vmax, ctypes.byref(wp), ctypes.byref(rp), 1, s[0].ctypes.data,
                                       s[1].ctypes.data, n_w, wthr_.ctypes.data_as(_lib.DP), n_r, rthr_.ctypes.data_as(_lib.DP),
                                       counts.ctypes.data, None, None)
        pairs = ctypes.c_int64()
        desc, nan_thr = np.array([2.0, 1.0]), np.array([1.0, math.nan])
        rejected = [dict(n_w=7, n_r=8), dict(n_w=32, n_r=1), dict(n_w=1, n_r=32), dict(n_w=64, n_r=64),     # the bin product
                    dict(n_w=0), dict(n_r=0), dict(n_w=65), dict(n_r=65),
                    dict(wthr_=desc), dict(rthr_=desc), dict(wthr_=nan_thr), dict(rthr_=nan_thr),
                    dict(dt_s=2 * DT), dict(wind=dict(dt_s=DT / 2)), dict(substeps=2), dict(wind=dict(substeps=3)),      # must agree
                    dict(vmax=None),
                    # the footprint's rules
                    dict(wind=dict(ck_cd=2.0)), dict(wind=dict(r_out_km=0.0)), dict(wind=dict(r_out_km=2001.0)),
                    dict(wind=dict(rmax_const_km=-1.0)), dict(wind=dict(substeps=65), substeps=65), dict(wind=dict(dt_s=0.0), dt_s=0.0),
                    # the rainfall's rules
                    dict(r_out_km=2001.0), dict(r_out_km=0.0), dict(stat=2), dict(v_lo_kt=0.0), dict(v_hi_kt=170.0),
                    dict(a=(math.nan,) + a0[1:]), dict(b=(3.96, 4.80, -14.0, -16.0)), dict(a=(-1.10, -6.0, 64.5, 150.0)),
                    dict(n_t_=0), dict(n_t_=n_t + 1)]
        for p in rejected:
            assert call(**p) == -1, p
            assert L.tcr_last_error(h).decode().startswith('tcr_compound:'), (p, L.tcr_last_error(h))
        assert call(n_w=7, n_r=8) == -1 and '(n_wbin + 1) * (n_rbin + 1) must be <= 64' in L.tcr_last_error(h).decode()
        assert call(substeps=2) == -1 and 'same dt_s and the same substeps' in L.tcr_last_error(h).decode()
        # none of them got as far as a launch: the context has still seen no compound call
        assert L.tcr_compound_pairs(h, ctypes.byref(pairs)) == -1
        assert call() == 0 and counts[0, 0, 0] == n_trk and counts[0, 0, :9].sum() > n_trk
        assert L.tcr_compound_pairs(h, ctypes.byref(pairs)) == 0 and pairs.value == n_trk * n_t
        assert call(n_w=7, n_r=7) == 0 and call(n_w=1, n_r=31) == 0 and call(n_w=31, n_r=1) == 0            # 64 cells
        assert call(stat=1) == 0 and call(wind=dict(ck_cd=1.0)) == 0 and call(wind=dict(r_out_km=100.0)) == 0
    finally:
        L.tcr_ctx_destroy(h)


@pytest.mark.gpu
def test_gpu_run_downscaling_tracks_then_cli(golden_env, built_lib, tmp_path):
    from tropical_cyclone_risk_amd import analysis, compound, compute, hazard, io as tio
    nl = TR._nl(start_year=2001, end_year=2003, tracks_per_year=40, dataset_type='SYNTHETIC', output_directory=str(tmp_path), exp_name='cp')
    os.makedirs(tmp_path / 'cp', exist_ok=True)
    fn = compute.run_downscaling('NA', env=golden_env, nl=nl)
    d = tio.read_tracks(fn)
    lon, lat, v, vmax = (np.asarray(d[k], float) for k in ('lon_trks', 'lat_trks', 'v_trks', 'vmax_trks'))
    env = [np.asarray(d[k], float) for k in analysis.ENV_VARS]
    dt = analysis.sample_spacing([d['time']])
    groups = np.asarray(d['tc_years']).astype(int) - 2001
    i = np.argwhere(np.isfinite(lon) & np.isfinite(vmax))[::53][:8]
    slon = np.concatenate([lon[i[:, 0], i[:, 1]] - 360.0, [-80.1918]])
    slat = np.concatenate([lat[i[:, 0], i[:, 1]] + 0.7, [25.7617]])
    sites = ['--site=%.12f,%.12f' % (a, b) for a, b in zip(slon, slat)]
    out = str(tmp_path / 'compound.npz')
    cmd = [sys.executable, '-m', 'tropical_cyclone_risk_amd.compound', fn, '--out', out, '--substeps', '4', '--wind-thresholds',
           '10:60:10', '--rain-thresholds', '5:75:10', '--wind-r-out-km', '300'] + sites
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert 'joint return period' in p.stdout and '(mm)' in p.stdout
    z = np.load(out)
    assert set(z.files) == {'counts', 'joint_return_period', 'either_return_period', 'wind_thresholds', 'rain_thresholds', 'site_lon',
                            'site_lat', 'total_years', 'wind_r_out_km', 'rain_r_out_km', 'substeps', 'stat', 'rmax_km', 'dt_s',
                            'group_file', 'group_year', 'files'}
    assert int(z['total_years']) == 3 and z['group_year'].tolist() == [2001, 2002, 2003] and int(z['substeps']) == 4
    assert str(z['stat']) == 'total' and float(z['dt_s']) == dt and float(z['wind_r_out_km']) == 300.0 and float(z['rain_r_out_km']) == 500.0
    wthr, rthr = np.arange(10.0, 61.0, 10.0), np.arange(5.0, 76.0, 10.0)
    assert np.array_equal(z['wind_thresholds'], wthr) and np.array_equal(z['rain_thresholds'], rthr)
    api = compound.site_compound(lon, lat, v, vmax, env, groups, z['site_lon'], z['site_lat'], dt, wthr, rthr, wind_r_out_km=300.0,
                                 substeps=4, n_groups=3)
    assert np.array_equal(z['counts'], api['counts']) and api['counts'][..., 1:, 1:].sum() > 0
    n_site = slon.size
    for key, table in (('joint_return_period', api['counts'][..., 1:, 1:]), ('either_return_period', CN.or_counts(api['counts']))):
        want = hazard.return_periods(table.reshape(n_site, 3, -1), 3).reshape(n_site, wthr.size, rthr.size)
        assert np.array_equal(z[key], want), key
    assert (z['either_return_period'] <= z['joint_return_period']).all()
    # the wind marginal is the footprint CLI's counts on the same thresholds
    wout = str(tmp_path / 'wind.npz')
    cmd = [sys.executable, '-m', 'tropical_cyclone_risk_amd.windfield', fn, '--out', wout, '--substeps', '4', '--thresholds', '10:60:10',
           '--r-out-km', '300'] + sites
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert np.array_equal(z['counts'][..., 1:, 0], np.load(wout)['counts'])
