"""Wind footprints (tropical_cyclone_risk_amd/windfield.py, csrc/tcr_windfield.hip): the peak wind of every storm at every site
from the Emanuel & Rotunno (2011) profile plus axi_to_max_wind's asymmetry.  CPU tests pin the NumPy restatement
(tests/windfield_numpy.py) to the reference's own vmax at every golden sample and to hand values, and check the argument
handling and the C struct layout; GPU tests (`-m gpu`) check the kernels against the restatement."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest

from tests import windfield_numpy as WN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DT = 3600.0


def _golden(basins=('NA', 'AU', 'GL')):
    """lon, lat, v, env (4 planes) [n][361] and the reference's vmax of the golden tracks."""
    lon, lat, v, env, vmax = [], [], [], [], []
    for b in basins:
        d = np.load(os.path.join(GOLDEN, 'tracks_%s.npz' % b))
        lon.append(d['traj'][:, 0]); lat.append(d['traj'][:, 1]); v.append(d['traj'][:, 2])
        env.append(np.moveaxis(d['envw'], 2, 0)); vmax.append(d['vmax'])
    return (np.concatenate(lon), np.concatenate(lat), np.concatenate(v), list(np.concatenate(env, axis=1)),
            np.concatenate(vmax))


def _nl(**over):
    from tropical_cyclone_risk_amd import namelist
    nl = types.SimpleNamespace(**{k: getattr(namelist, k) for k in dir(namelist) if not k.startswith('__')})
    for k, val in over.items():
        setattr(nl, k, val)
    return nl


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_reproduces_the_reference_vmax_at_every_golden_sample():
    """At r = rm on the maximising bearing the footprint is axi_to_max_wind's vmax; no azimuth of that ring exceeds it."""
    lon, lat, v, env, vmax = _golden()
    n = WN.track_length(lon, lat, v, env)
    rows = []
    for s in range(lon.shape[0]):
        k = int(n[s])
        if k < 2:
            assert np.isnan(vmax[s, :max(k, 1)]).all()      # one sample: no translation speed, no vmax
            continue
        ae, an, fac, mag = WN.asymmetry(lon[s, :k], lat[s, :k], v[s, :k], [e[s, :k] for e in env], DT)
        rows.append((lon[s, :k], lat[s, :k], v[s, :k], ae, an, fac * mag, vmax[s, :k]))
    assert len(rows) >= 50
    lo, la, vv, ae, an, amag, ref = (np.concatenate([r[i] for r in rows]) for i in range(7))
    assert np.isfinite(ref).all() and ref.size > 5000
    # the asymmetry is the reference's: v + fac |U| == vmax
    assert np.allclose(vv + amag, ref, rtol=1e-12, atol=0)
    rm = WN.willoughby_rmax_km(vv, la)
    h = np.where(la >= 0, 1.0, -1.0)
    an_, ae_ = np.where(amag > 0, an / np.where(amag > 0, amag, 1), 0), np.where(amag > 0, ae / np.where(amag > 0, amag, 1), 0)
    bearing = np.arctan2(h * an_, -h * ae_)              # d = h (A_n, -A_e) / |A|: t = h (-d_n, d_e) along A
    slon, slat = WN.direct(lo, la, rm, bearing)
    for c in (1.0, 0.5, 1.5):
        w, r = WN.wind(slon, slat, lo, la, vv, rm, ae, an, c)
        assert np.allclose(r, rm, rtol=1e-12, atol=0)
        err = np.abs(w / ref - 1)
        assert err.max() <= 1e-12, (c, err.max())
    for b in np.linspace(0, 2 * np.pi, 48, endpoint=False):
        rl, ra = WN.direct(lo, la, rm, bearing + b)
        w, _ = WN.wind(rl, ra, lo, la, vv, rm, ae, an, 1.0)
        assert (w <= ref * (1 + 1e-12)).all()
    assert (la < 0).sum() > 500 and (la > 0).sum() > 500      # both hemispheres


def test_profile_by_hand():
    c1 = dict(v=40.0, lat=0.0, c=1.0)                    # f = 0: V = 2 Mm r / (rm^2 + r^2), Mm = rm v
    rm = 30.0
    for r in (1.0, 15.0, 30.0, 60.0, 450.0):
        want = 2 * (rm * 1e3 * 40.0) * (r * 1e3) / ((rm * 1e3) ** 2 + (r * 1e3) ** 2)
        assert math.isclose(float(WN.profile(r, rm, c1['v'], c1['lat'], c1['c'])), want, rel_tol=1e-14)
    for c in (0.3, 0.5, 1.0, 1.5, 1.9):
        for lat in (-40.0, 0.0, 20.0):
            assert math.isclose(float(WN.profile(rm, rm, 50.0, lat, c)), 50.0, rel_tol=1e-13)        # V(rm) = v
    assert float(WN.profile(0.0, rm, 50.0, 20.0, 1.0)) == 0.0 and float(WN.profile(0.0, rm, 50.0, 20.0, 0.5)) == 0.0
    # large r: the f r^2 / 2 term wins, clamped to 0 (c = 1, f at 45 N, 1900 km)
    f = 2 * 7.292e-5 * math.sin(math.radians(45.0))
    r = 1.9e6
    assert 2 * (rm * 1e3 * 50 + f * (rm * 1e3) ** 2 / 2) * r / ((rm * 1e3) ** 2 + r ** 2) - f * r / 2 < 0
    assert float(WN.profile(1900.0, rm, 50.0, 45.0, 1.0)) == 0.0
    # c = 0.5 and 1.5 at a few x, f = 0
    for c, x, want in ((0.5, 2.0, (8 / 3.5) ** (1 / 1.5) / 2), (0.5, 0.5, (0.5 / 1.625) ** (1 / 1.5) / 0.5),
                       (1.5, 2.0, (8 / 6.5) ** 2 / 2), (1.5, 0.5, (0.5 / 0.875) ** 2 / 0.5), (1.5, 4.0, (32 / 24.5) ** 2 / 4)):
        got = float(WN.profile(x * rm, rm, 40.0, 0.0, c)) / 40.0      # V / v = ratio / x at f = 0
        assert math.isclose(got, want, rel_tol=1e-13), (c, x, got, want)


def test_willoughby_and_the_side_of_maximum_wind():
    assert WN.willoughby_rmax_km(0.0, 0.0) == 46.4
    assert math.isclose(float(WN.willoughby_rmax_km(50.0, -20.0)), 46.4 * math.exp(-0.775 + 0.338), rel_tol=1e-15)
    assert math.isclose(float(WN.willoughby_rmax_km(30.0, 35.0)), 46.4 * math.exp(-0.465 + 0.5915), rel_tol=1e-15)
    # a storm moving due east: maximum to the south (right of motion) in the NH, to the north (left) in the SH
    for lat0, want in ((20.0, 180.0), (-20.0, 0.0)):
        lon = 300.0 + 0.2 * np.arange(5)
        lat = np.full(5, lat0)
        v = np.full(5, 40.0)
        env = [np.zeros(5)] * 4
        ae, an, fac, mag = WN.asymmetry(lon, lat, v, env, DT)
        assert ae[2] > 0 and abs(an[2]) < 1e-12 * ae[2]
        rm = 30.0
        b = np.deg2rad(np.arange(0.0, 360.0, 1.0))
        sl, sa = WN.direct(lon[2], lat[2], rm, b)
        w, _ = WN.wind(sl, sa, lon[2], lat[2], v[2], rm, ae[2], an[2], 1.0)
        assert np.rad2deg(b[np.argmax(w)]) == want
        assert math.isclose(w.max(), 40.0 + fac[2] * mag[2], rel_tol=1e-12)
        assert math.isclose(w.min(), 40.0 - fac[2] * mag[2], rel_tol=1e-12)


def test_substeps_across_the_dateline():
    for lon_pair, want_d in (((179.5, -179.5), 1.0), ((359.8, 0.2), 0.4), ((-179.5, 179.5), -1.0)):
        lon = np.array([list(lon_pair)])
        lat, v = np.array([[10.0, 11.0]]), np.array([[30.0, 40.0]])
        env = [np.zeros((1, 2))] * 4
        rec = WN.samples(lon, lat, v, env, DT, rmax_km=20.0, substeps=4)[0]
        d = lon_pair[1] - lon_pair[0]
        d = d - 360.0 * np.floor((d + 180.0) / 360.0)
        assert math.isclose(d, want_d, rel_tol=1e-12)
        assert rec.shape == (6, 5)
        # the sub-samples step the short way round; the last one is the sample itself, in its own convention
        assert np.allclose(rec[0][:4], lon_pair[0] + d * np.array([0, 0.25, 0.5, 0.75]), rtol=0, atol=1e-12)
        assert rec[0][4] == lon_pair[1]
        assert np.allclose(rec[1], [10.0, 10.25, 10.5, 10.75, 11.0]) and np.allclose(rec[2], [30, 32.5, 35, 37.5, 40])
        assert np.allclose(rec[3], 20.0)
        # the midpoint is next to both samples, not on the other side of the globe
        _, r = WN.wind(lon_pair[0], 10.0, rec[0][2], rec[1][2], 35.0, 20.0, 0.0, 0.0, 1.0)
        assert r < 100.0
    # one-sample tracks and NaN tails
    lon = np.array([[1.0, np.nan, 3.0], [1.0, 2.0, 3.0]])
    env = [np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)), np.array([[0, 0, 0], [0, 0, np.nan]], float)]
    n = WN.track_length(lon, np.ones((2, 3)), np.ones((2, 3)), env)
    assert n.tolist() == [1, 2]
    rec = WN.samples(lon, np.ones((2, 3)), np.ones((2, 3)), env, DT, substeps=3)
    assert rec[0] is None and rec[1].shape == (6, 4)


def test_wind_struct_layout_matches_header():
    from tropical_cyclone_risk_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tcrisk_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
           'sizeof(tcr_wind_tracks),offsetof(tcr_wind_tracks, lon),offsetof(tcr_wind_tracks, rmax_km),'
           'offsetof(tcr_wind_tracks, n_group),offsetof(tcr_wind_tracks, group_off),sizeof(tcr_wind_params),'
           'offsetof(tcr_wind_params, rmax_const_km),offsetof(tcr_wind_params, substeps));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'sz.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 'sz')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    T, P = _lib.WindTracks, _lib.WindParams
    assert sizes == [ctypes.sizeof(T), T.lon.offset, T.rmax_km.offset, T.n_group.offset, T.group_off.offset, ctypes.sizeof(P),
                     P.rmax_const_km.offset, P.substeps.offset]


def test_windfield_symbols_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ('tcr_windfield_dev', 'tcr_windfield_host', 'tcr_windfield_pairs'):
        assert hasattr(L, name), name


def test_argument_errors_before_any_device_work():
    from tropical_cyclone_risk_amd import windfield
    rng = np.random.default_rng(0)
    lon, lat, v = 280 + rng.random((3, 5)), 20 + rng.random((3, 5)), 30 + rng.random((3, 5))
    env = [np.zeros((3, 5))] * 4
    g = np.zeros(3, np.int64)
    s = (np.array([280.0]), np.array([20.0]))
    base = dict(lon=lon, lat=lat, v=v, env=env, groups=g, site_lon=s[0], site_lat=s[1], dt_s=DT)
    bad = [dict(r_out_km=0.0), dict(r_out_km=2000.5), dict(r_out_km=np.nan), dict(substeps=0), dict(substeps=65),
           dict(substeps=1.5), dict(ck_cd=0.0), dict(ck_cd=2.0), dict(dt_s=0.0), dict(dt_s=np.inf),
           dict(thresholds=np.array([20.0, 10.0])), dict(thresholds=np.arange(65.0)), dict(thresholds=np.array([])),
           dict(thresholds=np.array([10.0, np.inf])), dict(rmax_km=0.0), dict(rmax_km=-5.0), dict(rmax_km=np.full((3, 4), 20.0)),
           dict(rmax_km=np.where(np.arange(5) == 3, 0.0, 20.0) * np.ones((3, 1))), dict(env=env[:3]),
           dict(v=v[:, :4]), dict(groups=np.zeros(2, np.int64)), dict(groups=np.array([0, -1, 0])), dict(site_lat=np.array([np.nan])),
           dict(site_lon=np.array([1.0, 2.0])), dict(groups=np.array([0, 1, 2]), n_groups=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            windfield.site_wind(**dict(base, **kw))
    # an rm plane is checked on the tracks only: past a track's end anything goes
    lon2 = lon.copy()
    lon2[0, 3] = np.nan
    lon2[1, 1] = np.nan
    assert windfield._track_length([lon2, lat, v] + env, np).tolist() == [3, 1, 5]


def test_cli_arguments():
    from tropical_cyclone_risk_amd import hazard, windfield
    a = windfield.parse_args(['x.nc', '--site=-80.19,25.76', '--grid', '270:271:0.5,20:21:1', '--rmax-km', '25',
                              '--r-out-km', '300', '--substeps', '4', '--thresholds', '20:60:10'])
    assert a.rmax_km == 25.0 and a.r_out_km == 300.0 and a.substeps == 4 and a.out == 'wind.npz'
    assert np.array_equal(a.thresholds, [20, 30, 40, 50, 60])
    lon, lat = hazard.collect_sites(a)
    assert lon.size == 7
    b = windfield.parse_args(['x.nc', '--site', '1,2'])
    assert b.rmax_km is None and b.ck_cd is None and b.r_out_km == 500.0 and b.substeps == 1
    assert np.array_equal(b.thresholds, hazard.DEFAULT_THRESHOLDS)
    with pytest.raises(SystemExit):
        windfield.parse_args(['x.nc'])


# ------------------------------------------------------------------------------------------------------------------ GPU
def _check(r, recs, groups, n_groups, slon, slat, r_out, c, thr):
    """site_max within the tolerance for some choice of the ambiguous decisions; counts consistent with it and with NumPy."""
    lo, amb_any, amb_vals = WN.site_max(recs, slon, slat, r_out, c)
    got = r['site_max']
    ok = WN.allowed(got, lo, amb_vals)
    assert ok.all(), [(int(i), int(s), got[i, s], lo[i, s]) for i, s in np.argwhere(~ok)[:5]]
    assert np.array_equal(r['counts'], WN.counts(got, groups, n_groups, thr))
    und = WN.undecided(lo, amb_any, thr)
    a, b = np.where(und, np.nan, got), np.where(und, np.nan, lo)
    assert np.array_equal(WN.counts(a, groups, n_groups, thr), WN.counts(b, groups, n_groups, thr))
    return lo, amb_any


def _stress_tracks(rng, n_trk=140, n_t=48):
    """Random walks of plausible storms: NH, SH, equatorial and dateline-crossing ones, both conventions, NaN tails in any of
    the seven planes, one-sample tracks."""
    lon0 = np.concatenate([rng.uniform(260, 340, 60), rng.uniform(175, 185, 30), rng.uniform(-3, 3, 10), rng.uniform(60, 120, 40)])
    lat0 = np.concatenate([rng.uniform(8, 35, 60), rng.uniform(-25, 25, 30), rng.uniform(-20, 20, 10), rng.uniform(-30, -2, 20),
                           rng.uniform(-1.5, 1.5, 20)])
    lon0, lat0 = lon0[:n_trk], lat0[:n_trk]
    step_lon = rng.normal(-0.15, 0.25, (n_trk, 1)) + rng.normal(0, 0.05, (n_trk, n_t))
    step_lat = rng.normal(0.1, 0.15, (n_trk, 1)) + rng.normal(0, 0.05, (n_trk, n_t))
    lon = lon0[:, None] + np.cumsum(step_lon, axis=1) - step_lon[:, :1]
    lat = np.clip(lat0[:, None] + np.cumsum(step_lat, axis=1) - step_lat[:, :1], -60, 60)
    conv = rng.random(n_trk) < 0.5
    lon[conv] = np.where(lon[conv] > 180, lon[conv] - 360, lon[conv])          # [-180, 180) for half of them
    v = np.clip(25 + np.cumsum(rng.normal(0.3, 1.5, (n_trk, n_t)), axis=1), -2, 85)
    env = [rng.normal(0, 8, (n_trk, n_t)) for _ in range(4)]
    end = rng.integers(1, n_t + 1, n_trk)
    end[:5] = 1                                                           # one-sample tracks
    end[5:40] = n_t
    planes = [lon, lat, v] + env
    for i in range(n_trk):
        if end[i] < n_t:
            planes[rng.integers(0, 7)][i, end[i]] = np.nan                 # a NaN in one plane ends the track ...
            if rng.random() < 0.5:
                for p in planes:                                          # ... and the reference writes NaN tails
                    p[i, end[i]:] = np.nan
    return lon, lat, v, env


def _stress_sites(rng, lon, lat, r_out, n_rand=60):
    live = np.argwhere(np.isfinite(lon) & np.isfinite(lat))
    pick = live[rng.choice(len(live), 150, replace=False)]
    cl, ca = lon[pick[:, 0], pick[:, 1]], lat[pick[:, 0], pick[:, 1]]
    el, ea = WN.direct(cl[:40], ca[:40], np.full(40, r_out), rng.uniform(0, 6.3, 40))            # at r_out
    nl_, na_ = WN.direct(cl[40:120], ca[40:120], rng.uniform(5, 1.3 * r_out, 80), rng.uniform(0, 6.3, 80))
    slon = np.concatenate([cl[120:], el, nl_, nl_[:20] + 360.0, nl_[20:40] - 360.0, rng.uniform(-180, 360, n_rand)])
    slat = np.concatenate([ca[120:], ea, na_, na_[:20], na_[20:40], rng.uniform(-50, 50, n_rand)])
    return slon, slat


def _groups(rng, n_trk):
    groups = np.zeros(n_trk, np.int64)
    groups[rng.choice(n_trk, 40, replace=False)] = 2
    groups[7] = 3
    rng.shuffle(groups)
    return groups, 5                                                      # groups 1 and 4 empty


@pytest.mark.gpu
def test_gpu_golden_tracks_on_a_site_grid(built_lib):
    from tropical_cyclone_risk_amd import windfield
    lon, lat, v, env, _ = _golden()
    n_trk = lon.shape[0]
    groups = np.arange(n_trk) % 3
    glon, glat = np.meshgrid(np.arange(-100.0, 361.0, 4.0), np.arange(-48.0, 49.0, 4.0))
    slon, slat = glon.ravel(), glat.ravel()
    thr = np.arange(10.0, 81.0, 5.0)
    recs = WN.samples(lon, lat, v, env, DT, substeps=2)
    r = windfield.site_wind(lon, lat, v, env, groups, slon, slat, DT, r_out_km=500.0, substeps=2, thresholds=thr, return_max=True)
    lo, _ = _check(r, recs, groups, 3, slon, slat, 500.0, 1.0, thr)
    assert (~np.isnan(lo)).sum() > 2000 and r['counts'].sum() > 500


@pytest.mark.gpu
def test_gpu_stress_matches_restatement(built_lib):
    from tropical_cyclone_risk_amd import windfield
    rng = np.random.default_rng(23)
    lon, lat, v, env = _stress_tracks(rng)
    n_trk, n_t = lon.shape
    groups, n_groups = _groups(rng, n_trk)
    rm_plane = rng.uniform(8.0, 90.0, (n_trk, n_t))
    cases = [(1, 1.0, None, 500.0), (3, 0.5, 35.0, 500.0), (6, 1.5, rm_plane, 300.0), (3, 1.0, rm_plane, 150.0),
             (1, 0.5, None, 800.0), (6, 1.0, 25.0, 500.0)]
    seen_amb = 0
    for sub, c, rm, r_out in cases:
        slon, slat = _stress_sites(rng, lon, lat, r_out)
        thr = np.sort(rng.uniform(0, 90, 12))
        recs = WN.samples(lon, lat, v, env, DT, rmax_km=rm, substeps=sub)
        r = windfield.site_wind(lon, lat, v, env, groups, slon, slat, DT, rmax_km=rm, ck_cd=c, r_out_km=r_out, substeps=sub,
                                thresholds=thr, return_max=True, n_groups=n_groups)
        lo, amb = _check(r, recs, groups, n_groups, slon, slat, r_out, c, thr)
        seen_amb += int(amb.sum())
        assert (r['counts'][:, 1] == 0).all() and (r['counts'][:, 4] == 0).all()
        assert np.isnan(r['site_max'][:, :5]).all()                     # one-sample tracks contribute nothing
        assert (~np.isnan(lo)).sum() > 100
    print('stress: %d (site, storm) pairs with an ambiguous sample' % seen_amb)


@pytest.mark.gpu
def test_gpu_bit_identical_across_runs_site_order_and_storm_order(built_lib):
    from tropical_cyclone_risk_amd import windfield
    rng = np.random.default_rng(5)
    lon, lat, v, env = _stress_tracks(rng)
    n_trk = lon.shape[0]
    groups, n_groups = _groups(rng, n_trk)
    slon, slat = _stress_sites(rng, lon, lat, 500.0)
    kw = dict(r_out_km=500.0, substeps=3, return_max=True, n_groups=n_groups)
    a = windfield.site_wind(lon, lat, v, env, groups, slon, slat, DT, **kw)
    b = windfield.site_wind(lon, lat, v, env, groups, slon, slat, DT, **kw)
    assert np.array_equal(a['site_max'].view(np.int64), b['site_max'].view(np.int64)) and np.array_equal(a['counts'], b['counts'])
    ps = rng.permutation(slon.size)
    c = windfield.site_wind(lon, lat, v, env, groups, slon[ps], slat[ps], DT, **kw)
    assert np.array_equal(c['site_max'].view(np.int64), a['site_max'][ps].view(np.int64))
    assert np.array_equal(c['counts'], a['counts'][ps])
    pt = rng.permutation(n_trk)                                          # storms shuffled within and across groups
    d = windfield.site_wind(lon[pt], lat[pt], v[pt], [e[pt] for e in env], groups[pt], slon, slat, DT, **kw)
    assert np.array_equal(d['site_max'].view(np.int64), a['site_max'][:, pt].view(np.int64))
    assert np.array_equal(d['counts'], a['counts'])


@pytest.mark.gpu
def test_gpu_host_and_device_entry_points_agree(built_lib):
    import torch
    from tropical_cyclone_risk_amd import windfield
    from tropical_cyclone_risk_amd.engine import TCEngine
    rng = np.random.default_rng(8)
    lon, lat, v, env = _stress_tracks(rng)
    n_trk, n_t = lon.shape
    groups, n_groups = _groups(rng, n_trk)
    slon, slat = _stress_sites(rng, lon, lat, 400.0)
    rm = rng.uniform(10.0, 60.0, (n_trk, n_t))
    kw = dict(rmax_km=rm, ck_cd=1.5, r_out_km=400.0, substeps=4, return_max=True, n_groups=n_groups)
    ref = windfield.site_wind(lon, lat, v, env, groups, slon, slat, DT, **kw)
    dev = torch.device('cuda', 0)
    t = [torch.as_tensor(x, device=dev) for x in [lon, lat, v] + env + [slon, slat, rm]]
    eng = TCEngine('NA', device=0)
    side = torch.cuda.Stream(dev)
    try:
        for _ in range(2):
            with torch.cuda.stream(side):
                r = windfield.site_wind(t[0], t[1], t[2], t[3:7], groups, t[7], t[8], DT, engine=eng,
                                        **dict(kw, rmax_km=t[9]))
            side.synchronize()
            assert r['counts'].device == dev and r['site_max'].device == dev
            assert np.array_equal(r['counts'].cpu().numpy(), ref['counts'])
            assert np.array_equal(r['site_max'].cpu().numpy().view(np.int64), ref['site_max'].view(np.int64))
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
        planes = [np.full((n_trk, n_t), x) for x in (280.0, 20.0, 30.0, 1.0, 1.0, 0.0, 0.0)]
        planes[0] = planes[0] + 0.1 * np.arange(n_t)
        rm = np.full((n_trk, n_t), 20.0)
        rm[1, 2] = -1.0
        off = (ctypes.c_int64 * 2)(0, n_trk)
        s = np.array([280.2]), np.array([20.0])
        thr = np.array([10.0, 20.0])
        counts = np.zeros((1, 1, 2), np.int32)

        def call(rmax=None, **p):
            trk = _lib.WindTracks(n_trk=n_trk, n_t=n_t, row_stride=n_t, lon=planes[0].ctypes.data, lat=planes[1].ctypes.data,
                                  v=planes[2].ctypes.data, u250=planes[3].ctypes.data, v250=planes[4].ctypes.data,
                                  u850=planes[5].ctypes.data, v850=planes[6].ctypes.data,
                                  rmax_km=rmax.ctypes.data if rmax is not None else None, n_group=1, group_off=off)
            prm = _lib.WindParams(**dict(dict(dt_s=DT, ck_cd=1.0, r_out_km=500.0, rmax_const_km=0.0, substeps=1), **p))
            return L.tcr_windfield_host(h, ctypes.byref(trk), ctypes.byref(prm), 1, s[0].ctypes.data, s[1].ctypes.data, 2,
                                        thr.ctypes.data_as(_lib.DP), counts.ctypes.data, None)
        assert call() == 0 and counts.sum() > 0
        for p in (dict(r_out_km=2001.0), dict(substeps=65), dict(ck_cd=2.0), dict(dt_s=0.0), dict(rmax_const_km=-1.0)):
            assert call(**p) == -1, p
        assert call(rm) == -1 and b'rmax_km' in L.tcr_last_error(h)
        assert call(np.full((n_trk, n_t), 20.0), rmax_const_km=5.0) == -1
        assert call(np.full((n_trk, n_t), 20.0)) == 0
        pairs = ctypes.c_int64()
        assert L.tcr_windfield_pairs(h, ctypes.byref(pairs)) == 0 and pairs.value > 0
    finally:
        L.tcr_ctx_destroy(h)


def _run_downscaling(golden_env, tmp_path):
    from tropical_cyclone_risk_amd import compute
    nl = _nl(start_year=2001, end_year=2003, tracks_per_year=40, dataset_type='SYNTHETIC', output_directory=str(tmp_path),
             exp_name='wf')
    os.makedirs(tmp_path / 'wf', exist_ok=True)
    return compute.run_downscaling('NA', env=golden_env, nl=nl)


@pytest.mark.gpu
def test_gpu_run_downscaling_tracks_then_cli(golden_env, built_lib, tmp_path):
    from tropical_cyclone_risk_amd import hazard, io as tio, windfield
    from tropical_cyclone_risk_amd.climatology import sample_spacing
    fn = _run_downscaling(golden_env, tmp_path)
    d = tio.read_tracks(fn)
    lon, lat, v, vmax = (np.asarray(d[k], float) for k in ('lon_trks', 'lat_trks', 'v_trks', 'vmax_trks'))
    env = [np.asarray(d[k], float) for k in windfield.ENV_VARS]
    dt = sample_spacing([d['time']])
    # the restatement's v + fac |U| is the file's vmax_trks at every sample: the footprint's asymmetry is the pipeline's
    n = WN.track_length(lon, lat, v, env)
    checked = 0
    for s in range(lon.shape[0]):
        k = int(n[s])
        if k < 2:
            continue
        _, _, fac, mag = WN.asymmetry(lon[s, :k], lat[s, :k], v[s, :k], [e[s, :k] for e in env], dt)
        assert np.allclose(v[s, :k] + fac * mag, vmax[s, :k], rtol=1e-12, atol=0), s
        checked += k
    assert checked > 1000
    groups = np.asarray(d['tc_years']).astype(int) - 2001
    i = np.argwhere(np.isfinite(lon))[::53][:8]
    slon = np.concatenate([lon[i[:, 0], i[:, 1]] - 360.0, [-80.1918]])
    slat = np.concatenate([lat[i[:, 0], i[:, 1]] + 0.7, [25.7617]])
    thr = np.arange(10.0, 81.0, 5.0)
    for sub in (1, 4):
        recs = WN.samples(lon, lat, v, env, dt, substeps=sub)
        r = windfield.site_wind(lon, lat, v, env, groups, slon, slat, dt, substeps=sub, thresholds=thr, return_max=True, n_groups=3)
        _check(r, recs, groups, 3, slon, slat, 500.0, 1.0, thr)
    # CLI -> npz equals the API
    out = str(tmp_path / 'wind.npz')
    cmd = [sys.executable, '-m', 'tropical_cyclone_risk_amd.windfield', fn, '--out', out, '--substeps', '4']
    cmd += ['--site=%.12f,%.12f' % (a, b) for a, b in zip(slon, slat)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert 'return period' in p.stdout
    z = np.load(out)
    assert set(z.files) == {'counts', 'return_period', 'thresholds', 'site_lon', 'site_lat', 'total_years', 'r_out_km', 'substeps',
                            'rmax_km', 'dt_s', 'group_file', 'group_year', 'files'}
    assert int(z['total_years']) == 3 and z['group_year'].tolist() == [2001, 2002, 2003] and int(z['substeps']) == 4
    assert np.allclose(z['site_lon'], slon, rtol=0, atol=1e-11) and np.allclose(z['site_lat'], slat, rtol=0, atol=1e-11)
    api = windfield.site_wind(lon, lat, v, env, groups, z['site_lon'], z['site_lat'], dt, substeps=4, n_groups=3)
    assert np.array_equal(z['counts'], api['counts']) and api['counts'].sum() > 0
    assert np.array_equal(z['return_period'], hazard.return_periods(api['counts'], 3))
